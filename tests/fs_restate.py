"""A restatement of canu's falconsense (src/correction/falconsense.C, falconConsensus*.C and the
edlib calls they make) in Python, for the tests of canu_amd.falconsense.

Edit distances are Myers' bit-vector recurrence with one Python integer per column (the whole
query is one word), so a 4 kb x 5 kb pass takes some tens of milliseconds.  edlib's results are
restated in closed form -- distance, first best end, longest start, and the path by the
leaf / Hirschberg recursion of obtainAlignment (edlib.C:1164-1404) -- and pinned to the
reference binary by the fixtures tests/golden/fs_*.npz (tests/test_fs_cpu.py).

`consensus` keeps the reference's doubles (DBL_MIN included); `consensus_int` is the integer
form the device uses: every score is a multiple of 0.5, so twice the score is an exact integer,
and DBL_MIN -- the smallest positive double, which disappears in any sum with a nonzero
multiple of 0.5 and is not greater than itself -- is 0.
"""
from __future__ import annotations

import math
import re
import struct
import sys

import numpy as np

MATCH, INSERT, DELETE, MISMATCH = 0, 1, 2, 3         # EDLIB_EDOP_*
DBL_MIN = sys.float_info.min
MIN_EVIDENCE = 500                                    # falconConsensus-alignTag.C:144
LEAF_BYTES = 1024 * 1024                              # edlib.C:1193
U16MAX = 65535

_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(b: bytes) -> bytes:
    return b.translate(_COMP)[::-1]


def new_log() -> dict:
    return {"leaf": 0, "split": 0, "max_depth": 0, "rejected": 0, "skipped": 0, "truncated": 0,
            "aligned": 0, "tie_first_appearance": 0, "n_link": 0, "dropped_first": 0,
            "empty_output": 0, "split_top": 0, "split_bottom": 0, "empty_side": 0, "cells": 0}


# ------------------------------------------------------------------ Myers, one word per column

def _peq(q: bytes) -> dict:
    a = np.frombuffer(q, dtype=np.uint8)
    out = {}
    for c in np.unique(a):
        bits = np.packbits(a == c, bitorder="little")
        out[int(c)] = int.from_bytes(bits.tobytes(), "little")
    return out


def myers(q: bytes, t: bytes, top: int, keep: bool = False):
    """The matrix of q (rows) against t (columns); top 0 lets an alignment start at any column
    (HW), 1 charges every target base before it (SHW, NW).  -> (bottom row, Pv, Mv of the last
    column, [(Pv, Mv) per column] if keep)."""
    m = len(q)
    mask = (1 << m) - 1
    hb = 1 << (m - 1)
    peq = _peq(q)
    Pv, Mv, sc = mask, 0, m
    bottom, cols = [], []
    for c in t:
        Eq = peq.get(c, 0)
        Xv = Eq | Mv
        Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq
        Ph = Mv | (~(Xh | Pv) & mask)
        Mh = Pv & Xh
        if Ph & hb:
            sc += 1
        elif Mh & hb:
            sc -= 1
        Ph = ((Ph << 1) | top) & mask
        Mh = (Mh << 1) & mask
        Pv = Mh | (~(Xv | Ph) & mask)
        Mv = Ph & Xv
        bottom.append(sc)
        if keep:
            cols.append((Pv, Mv))
    return bottom, Pv, Mv, cols


def _bits(x: int, m: int) -> np.ndarray:
    return np.unpackbits(np.frombuffer(x.to_bytes((m + 7) // 8, "little"), dtype=np.uint8),
                         bitorder="little")[:m].astype(np.int32)


def column_scores(Pv: int, Mv: int, m: int, top: int) -> np.ndarray:
    """Scores of rows 0..m-1 of a column whose boundary row holds `top`."""
    return top + np.cumsum(_bits(Pv, m) - _bits(Mv, m))


def locate(q: bytes, t: bytes, k: int, log: dict | None = None):
    """edlibAlign(q, t, k, EDLIB_MODE_HW): -> (distance, start, end) or None (edlib.C:193-236)."""
    bottom, _, _, _ = myers(q, t, 0)
    best = min(bottom)
    if log is not None:
        log["cells"] += len(q) * len(t)
    if best > k:
        return None
    end = bottom.index(best)
    rb, _, _, _ = myers(q[::-1], t[:end + 1][::-1], 1)
    if log is not None:
        log["cells"] += len(q) * (end + 1)
    last = max(i for i, s in enumerate(rb) if s == best)
    return best, end - last, end


def is_leaf(qlen: int, tlen: int) -> bool:
    nb = (qlen + 63) // 64
    return 20 * nb * tlen + 8 * tlen < LEAF_BYTES


def leaf_path(q: bytes, t: bytes, best: int) -> bytes:
    """obtainAlignmentTraceback (edlib.C:945-1145): up if it costs one, else left if it costs
    one, else the diagonal; at a boundary the rest is flushed."""
    m, n = len(q), len(t)
    _, _, _, cols = myers(q, t, 1, keep=True)
    M = np.empty((m + 1, n + 1), dtype=np.int32)
    M[:, 0] = np.arange(m + 1)
    M[0, :] = np.arange(n + 1)
    for c, (Pv, Mv) in enumerate(cols):
        M[1:, c + 1] = column_scores(Pv, Mv, m, c + 1)
    assert int(M[m, n]) == best, (int(M[m, n]), best)
    ops = bytearray()
    r, c = m, n
    while r > 0 and c > 0:
        cur = int(M[r, c])
        if int(M[r - 1, c]) + 1 == cur:
            ops.append(INSERT)
            r -= 1
        elif int(M[r, c - 1]) + 1 == cur:
            ops.append(DELETE)
            c -= 1
        else:
            ops.append(MATCH if int(M[r - 1, c - 1]) == cur else MISMATCH)
            r -= 1
            c -= 1
    ops += bytes([INSERT]) * r + bytes([DELETE]) * c
    ops.reverse()
    return bytes(ops)


def path(q: bytes, t: bytes, best: int, log: dict, depth: int = 0) -> bytes:
    """obtainAlignment (edlib.C:1164-1404)."""
    m, n = len(q), len(t)
    if m == 0 or n == 0:
        log["empty_side"] += 1
        return bytes([DELETE if m == 0 else INSERT]) * (m + n)
    if is_leaf(m, n):
        log["leaf"] += 1
        log["cells"] += m * n
        return leaf_path(q, t, best)
    log["split"] += 1
    log["max_depth"] = max(log["max_depth"], depth + 1)
    log["cells"] += m * n
    lw = n // 2
    rw = n - lw
    _, Pv, Mv, _ = myers(q, t[:lw], 1)
    L = column_scores(Pv, Mv, m, lw)
    _, Pv, Mv, _ = myers(q[::-1], t[lw:][::-1], 1)
    R = column_scores(Pv, Mv, m, rw)[::-1]            # R[r] = ED(q[r:], t[lw:])
    hit = np.nonzero(L[:-1] + R[1:] == best)[0]
    if hit.size:
        r = int(hit[0])
        ls, rs = int(L[r]), int(R[r + 1])
    elif lw + int(R[0]) == best:
        log["split_top"] += 1
        r, ls, rs = -1, lw, int(R[0])
    elif int(L[m - 1]) + rw == best:
        log["split_bottom"] += 1
        r, ls, rs = m - 1, int(L[m - 1]), rw
    else:
        raise AssertionError("no split row")
    return path(q[:r + 1], t[:lw], ls, log, depth + 1) + path(q[r + 1:], t[lw:], rs, log, depth + 1)


# ------------------------------------------------------------------ tags

def align_tags(ops: bytes, q: bytes, tbgn: int) -> list:
    """alignReadsToTemplate's gap strip (:203-219) and getAlignTags (:72-116):
    (t_pos, delta, q_base, p_t_pos, p_delta, p_q_base), bases as byte values."""
    f, l = 0, len(ops)
    while f < l and ops[f] == INSERT:
        f += 1
    while l > f and ops[l - 1] == INSERT:
        l -= 1
    i, j = f - 1, tbgn - 1
    p_j, jj, p_jj, p_b = -1, 0, 0, ord(".")
    tags = []
    for op in ops[f:l]:
        if op != DELETE:
            i += 1
            jj += 1
            qb = q[i]
        else:
            qb = ord("-")
        if op != INSERT:
            j += 1
            jj = 0
        if jj >= U16MAX or p_jj >= U16MAX:
            continue
        tags.append((j, jj, qb, p_j, p_jj, p_b))
        p_j, p_jj, p_b = j, jj, qb
    return tags


def window(ev_len: int, bgn: int, end: int, tlen: int) -> tuple[int, int]:
    """falconConsensus-alignTag.C:149-163."""
    expansion = int((1.4 * ev_len - (end - bgn)) / 2)
    if expansion > 0:
        bgn -= expansion
        end += expansion
    return max(bgn, 0), min(end, tlen)


def align_evidence(template: bytes, evidence: list, min_identity: float, log: dict):
    """alignReadsToTemplate: evidence is [(bases, placed_bgn, placed_end)], the template first.
    -> (one tag list or None per evidence read, [aligned, skipped, rejected])."""
    max_diff = 1.0 - min_identity
    tlen = len(template)
    out = []
    counts = [0, 0, 0]
    for seq, pb, pe in evidence:
        if len(seq) > tlen:
            seq = seq[:tlen]
            log["truncated"] += 1
        if len(seq) < MIN_EVIDENCE:
            log["skipped"] += 1
            counts[1] += 1
            out.append(None)
            continue
        tol = int(math.ceil(min(len(seq), tlen) * max_diff * 1.1))
        assert pe > pb
        wb, we = window(len(seq), pb, pe, tlen)
        res = locate(seq, template[wb:we], tol, log)
        # alignDiff = editDistance / (double)(end - start): the divisor is one short of the span
        if res is not None and res[2] == res[1]:
            res = None if res[0] > 0 else res         # x / 0.0 is inf, and inf >= maxDifference
        elif res is not None and res[0] / float(res[2] - res[1]) >= max_diff:
            res = None
        if res is None:
            log["rejected"] += 1
            counts[2] += 1
            out.append(None)
            continue
        dist, start, end = res
        ops = path(seq, template[wb + start:wb + end + 1], dist, log)
        out.append(align_tags(ops, seq, wb + start))
        log["aligned"] += 1
        counts[0] += 1
    return out, counts


# ------------------------------------------------------------------ consensus

_SLOT = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def _columns(tag_lists: list, tlen: int, log: dict):
    cov = np.zeros(tlen, dtype=np.int64)
    cols: dict = {}                                    # (t_pos, delta, slot) -> [[pi, pj, pc, n]]
    for tags in tag_lists:
        if tags is None:
            continue
        for (j, jj, qb, p_j, p_jj, p_b) in tags:
            if jj == 0:
                cov[j] += 1
            links = cols.setdefault((j, jj, _SLOT.get(qb, 4)), [])
            for ln in links:
                if ln[0] == p_j and ln[1] == p_jj and ln[2] == p_b:
                    ln[3] += 1
                    break
            else:
                links.append([p_j, p_jj, p_b, 1])
                if p_b == ord("N"):
                    log["n_link"] += 1
    return cov, cols


def _backtrack(best_key, first_ck: int, back: dict, cov, tlen: int, min_cov: int,
               log: dict) -> bytes:
    """The walk back from the best column.  The letter of that first column is chosen by
    g_best_ck, which the scan sets to the *index of the best link* in the column's list, not to
    the column's base (falconConsensus.C:232-236, :253, :267-273): link 0 writes A, 1 C, 2 G,
    3 T, and a later one nothing."""
    out = bytearray()
    key = best_key
    first = True
    while True:
        i, _, ck = key
        if first:
            ck = min(first_ck, 4)
            first = False
        bb = b"-" if ck == 4 else (b"acgt" if cov[i] <= min_cov else b"ACGT")[ck:ck + 1]
        prev = back[key]
        if prev is None or len(out) >= 2 * tlen:
            if prev is None:
                log["dropped_first"] += 1
            break
        key = prev
        if bb != b"-":
            out += bb
    out.reverse()
    return bytes(out)


def consensus(tag_lists: list, tlen: int, min_cov: int, log: dict | None = None) -> bytes:
    """falconConsensus::getConsensus in the reference's doubles.  No column above DBL_MIN (where
    the reference asserts) gives b""."""
    log = new_log() if log is None else log
    cov, cols = _columns(tag_lists, tlen, log)
    score: dict = {}
    back: dict = {}
    g_best, g_key = DBL_MIN, None
    for key in sorted(cols):
        best, bprev, bck = DBL_MIN, None, 0           # a best link without predecessor ends
        for ck, (pi, pj, pc, n) in enumerate(cols[key]):   # the path as a column without links
            s = n - cov[key[0]] * 0.5
            if pi != -1:
                s += score[(pi, pj, _SLOT.get(pc, 4))]
            if s > best:
                best, bprev, bck = s, (None if pi == -1 else (pi, pj, _SLOT.get(pc, 4))), ck
            elif s == best and s > DBL_MIN:
                log["tie_first_appearance"] += 1
        score[key] = best
        back[key] = bprev
        if best > g_best:
            g_best, g_key, g_ck = best, key, bck
    if g_key is None:
        return b""
    return _backtrack(g_key, g_ck, back, cov, tlen, min_cov, log)


def consensus_int(tag_lists: list, tlen: int, min_cov: int) -> bytes:
    """The same scan with twice the score in integers and DBL_MIN as 0."""
    log = new_log()
    cov, cols = _columns(tag_lists, tlen, log)
    score: dict = {}
    back: dict = {}
    g_best, g_key = 0, None
    for key in sorted(cols):
        best, bprev, bck = 0, None, 0
        for ck, (pi, pj, pc, n) in enumerate(cols[key]):
            s = 2 * n - int(cov[key[0]])
            if pi != -1:
                s += score[(pi, pj, _SLOT.get(pc, 4))]
            if s > best:
                best, bprev, bck = s, (None if pi == -1 else (pi, pj, _SLOT.get(pc, 4))), ck
        score[key] = best
        back[key] = bprev
        if best > g_best:
            g_best, g_key, g_ck = best, key, bck
    if g_key is None:
        return b""
    return _backtrack(g_key, g_ck, back, cov, tlen, min_cov, log)


# ------------------------------------------------------------------ the program

def pieces(cns: bytes, min_output_length: int) -> list:
    """strtok(seq, "acgt") and the strict length test (falconsense.C:164-188)."""
    return [p for p in re.split(rb"[acgt]+", cns) if len(p) > min_output_length]


def fasta_record(tig_id: int, k: int, seq: bytes) -> bytes:
    """AS_UTL_writeFastA(F, seq, len, 60, ">read%u_%d\\n")."""
    body = b"".join(seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60))
    return b">read%d_%d\n" % (tig_id, k) + body


def evidence_of(reads: dict, tig_id: int, children) -> list:
    """generateFalconConsensus' evidence list: the template, then every child oriented and
    trimmed.  children: rows of (ident, reverse, min, max, askip, bskip)."""
    t = reads[tig_id]
    ev = [(t, 0, len(t))]
    for (ident, rev, mn, mx, askip, bskip) in children:
        s = reads[int(ident)]
        if rev:
            s = revcomp(s)
        s = s[int(askip):len(s) - int(bskip)]
        ev.append((s, int(mn), int(mx)))
    return ev


def correct_tig(reads: dict, tig_id: int, children, min_cov: int, min_identity: float,
                log: dict | None = None, integer: bool = False):
    """-> (consensus with its lower case, [aligned, skipped, rejected])."""
    log = new_log() if log is None else log
    t = reads[tig_id]
    tags, counts = align_evidence(t, evidence_of(reads, tig_id, children), min_identity, log)
    if all(x is None for x in tags):
        return b"", counts
    if integer:
        return consensus_int(tags, len(t), min_cov), counts
    return consensus(tags, len(t), min_cov, log), counts


def atoi(s: str) -> int:
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def parse_args(argv: list) -> dict:
    """falconsense.C:229-270; -ci goes through atoi, as there."""
    o = {"gkp": None, "cor": None, "prefix": None, "threads": 1, "bgn": 0, "end": 0xFFFFFFFF,
         "list": None, "cc": 4, "cl": 500, "ci": 0.5}
    i = 0
    while i < len(argv):
        a = argv[i]
        key = {"-G": "gkp", "-C": "cor", "-p": "prefix", "-r": "list"}.get(a)
        num = {"-t": "threads", "-b": "bgn", "-e": "end", "-cc": "cc", "-cl": "cl", "-ci": "ci"}.get(a)
        if key:
            i += 1
            o[key] = argv[i]
        elif num:
            i += 1
            o[num] = atoi(argv[i]) & 0xFFFFFFFF if num in ("bgn", "end", "cc", "cl") else atoi(argv[i])
        else:
            raise ValueError(f"unknown option '{a}'")
        i += 1
    o["ci"] = float(o["ci"])
    return o


def selected(o: dict, num_reads: int, read_list) -> list:
    """The tigs main() processes (falconsense.C:314-340): idMin <= ii < idMax, idMax clamped to
    the read count -- so read -e itself is left out -- and the -r list, itself cut to
    [idMin, idMax]."""
    bgn, end = o["bgn"], min(o["end"], num_reads)
    keep = {i for i in (read_list or []) if bgn <= i <= end}
    return [ii for ii in range(bgn, end) if not keep or ii in keep]


def falconsense(reads: dict, layouts, children, argv: list, read_list=None, log=None):
    """The program: layouts are rows of (tig_id, layout_len, first_child, n_children) for every
    tig of the store.  -> (stdout, stderr)."""
    o = parse_args(argv)
    log = new_log() if log is None else log
    by_id = {int(l[0]): l for l in layouts}
    out, err = bytearray(), bytearray()
    for ii in selected(o, len(reads), read_list):
        _, llen, first, n = (int(v) for v in by_id[ii])
        err += b"Processing read %d of length %d with %d evidence reads.\n" % (ii, llen, n)
        cns, _ = correct_tig(reads, ii, children[first:first + n], o["cc"], o["ci"], log)
        k = 0
        for p in pieces(cns, o["cl"]):
            err += b"Generated read %d_%d of length %d.\n" % (ii, k, len(p))
            out += fasta_record(ii, k, p)
            k += 1
        if k == 0:
            log["empty_output"] += 1
    return bytes(out), bytes(err)


# ------------------------------------------------------------------ the corStore

TIG_RECORD = struct.Struct("<I4xddIIIII4x")           # tgTigRecord, 48 bytes
STORE_ENTRY_BYTES = TIG_RECORD.size + 8               # tgStoreEntry
POSITION = np.dtype([("ident", "<u4"), ("flags", "<u4"), ("anchor", "<u4"), ("ahang", "<i4"),
                     ("bhang", "<i4"), ("askip", "<i4"), ("bskip", "<i4"), ("min", "<i4"),
                     ("max", "<i4"), ("delta_offset", "<u4"), ("delta_len", "<u4")])
MASR_MAGIC = 0x5253414D

LAYOUT_DTYPE = np.dtype([("tig_id", "<u4"), ("layout_len", "<u4"), ("first_child", "<u4"),
                         ("n_children", "<u4")])
CHILD_DTYPE = np.dtype([("ident", "<u4"), ("reverse", "<u4"), ("min", "<i4"), ("max", "<i4"),
                        ("askip", "<i4"), ("bskip", "<i4")])


def decode_corstore(tig: bytes, dat: bytes):
    """seqDB.v001.tig and seqDB.v001.dat -> (layouts, children) of every tig not deleted."""
    magic, version, total, indx, n = struct.unpack_from("<IIIII", tig, 0)
    if magic != MASR_MAGIC or version != 1 or len(tig) != 20 + n * STORE_ENTRY_BYTES:
        raise ValueError("not a version 1 tig index")
    lay, kids = [], []
    for k in range(n):
        base = 20 + k * STORE_ENTRY_BYTES
        (word,) = struct.unpack_from("<Q", tig, base + TIG_RECORD.size)
        if (word >> 13) & 1:                          # isDeleted
            continue
        off = word >> 24
        if dat[off:off + 4] != b"TIGR":
            raise ValueError(f"tig {k}: no record at {off}")
        tid, _, _, _, llen, glen, nch, _ = TIG_RECORD.unpack_from(dat, off + 4)
        p = np.frombuffer(dat, dtype=POSITION, count=nch, offset=off + 4 + TIG_RECORD.size + 2 * glen)
        lay.append((tid, llen, len(kids), nch))
        kids += [(int(c["ident"]), (int(c["flags"]) >> 3) & 1, int(c["min"]), int(c["max"]),
                  int(c["askip"]), int(c["bskip"])) for c in p]
    return np.array(lay, dtype=LAYOUT_DTYPE), np.array(kids, dtype=CHILD_DTYPE)


# ------------------------------------------------------------------ fixtures

FIXTURES = ["a", "b", "c", "d", "e", "f", "g"]
# evidence reads aligned, skipped and rejected over each fixture's selected tigs, templates
# included, as this restatement counts them (tests/test_fs_cpu.py holds it to that)
EXPECTED_COUNTS = {"a": (66, 0, 0), "b": (62, 0, 0), "c": (56, 0, 0), "d": (46, 1, 0),
                   "e": (14, 0, 0), "f": (104, 0, 0), "g": (7, 1, 1)}


def golden(name: str) -> dict:
    """tests/golden/fs_<name>.npz (tools/make_fs_golden.py)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"fs_{name}.npz"))
    reads = {i + 1: z["bases"][int(o):int(o) + int(n)].tobytes()
             for i, (o, n) in enumerate(zip(z["offsets"], z["lengths"]))}
    return {"bases": z["bases"], "offsets": z["offsets"], "lengths": z["lengths"], "reads": reads,
            "tig": z["tig"].tobytes(), "dat": z["dat"].tobytes(), "layouts": z["layouts"],
            "children": z["children"], "args": z["args"].tobytes().decode().split(),
            "read_list": [int(i) for i in z["read_list"]] or None,
            "stdout": z["stdout"].tobytes(), "stderr": z["stderr"].tobytes()}


def run_golden(g: dict, log: dict | None = None):
    return falconsense(g["reads"], [tuple(l) for l in g["layouts"]],
                       [tuple(k) for k in g["children"]], g["args"], g["read_list"], log)
