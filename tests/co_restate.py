"""A Python restatement of canu's correctOverlaps (src/overlapErrorAdjustment/), the checker of the
GPU library on inputs the reference was not run on.  tests/test_co_cpu.py pins it to the
reference's own .oea bytes and counters (tests/golden/co_*.npz, tools/make_co_golden.py).

Bases are codes 0..3 = acgt; every byte outside ACGTacgt is 'a' (correctOverlaps-Correct_Frags.C:
200-206).  Edit_Match_Limit is findErrors' table (fe_restate.match_limit; correctOverlaps.C:
131-133 makes the same call).  `branches`, where given, counts which paths ran.
"""
from __future__ import annotations

import math
import os
import struct

import numpy as np

import fe_restate as FR
from fe_restate import (A_INSERT, A_SUBST, DELETE, IDENT, RED_DTYPE, T_INSERT, T_SUBST,  # noqa: F401
                        filter_read, make_record, match_limit, unpack_olap)

BRANCH_PT_MATCH_VALUE = 0.272           # correctOverlaps.H:51
AS_MAX_EVALUE = 4095                    # ovOverlap.H:41-42
EVALUE_SHIFT = 42

COUNTERS = ("olaps_fwd", "olaps_rev", "total", "failed_both", "failed_either", "failed_end",
            "failed_length", "rha_fail", "rha_pass")
CORRECTED = ("corrected_bases", "substitutions", "deletions", "insertions")
# the branches the fixtures must reach (test_co_cpu.py)
REQUIRED_BRANCHES = ("trim_a_stop", "trim_a_short", "trim_b_stop", "trim_b_short",
                     "insert_copy", "insert_after_subst", "fail_end", "fail_length", "fail_both",
                     "rev_adjust", "hang_a", "hang_b_fwd", "hang_b_rev") + tuple(
    f"at_{w}_{t}" for w in ("a", "b_fwd", "b_rev") for t in ("m1", "0", "p1"))


class BadInput(ValueError):
    """Where the reference asserts or reads outside its arrays."""


def _bump(branches, key):
    if branches is not None:
        branches[key] = branches.get(key, 0) + 1


def _probe(branches, which, hang, adjust):
    """Counts a hang that lands one short of, on, or one past an entry's adjpos."""
    if branches is not None:
        pos = {p for p, _ in adjust}
        for d, tag in ((-1, "m1"), (0, "0"), (1, "p1")):
            if hang - d in pos:
                _bump(branches, f"at_{which}_{tag}")


def encode_evalue(q: float) -> int:
    """AS_OVS_encodeEvalue, ovOverlap.H:44-45."""
    return int(10000.0 * q + 0.5) if q < AS_MAX_EVALUE / 10000.0 else AS_MAX_EVALUE


def evalue_of(rec) -> int:
    return (int(rec["w0"]) >> EVALUE_SHIFT) & 0xFFF


def with_evalue(rec: tuple, ev: int) -> tuple:
    a, b, w0, w1 = rec
    return (a, b, (w0 & ~(0xFFF << EVALUE_SHIFT)) | ((ev & 0xFFF) << EVALUE_SHIFT), w1)


def error_bound(i: int, erate: float) -> int:
    """correctOverlaps.C:135-136."""
    return int(math.ceil(i * erate))


# ------------------------------------------------------------------------- the corrections

def correct_read(cur_id: int, oseq: np.ndarray, C: np.ndarray, cpos: int, changes=None,
                 branches=None):
    """correctRead, correctOverlaps-Correct_Frags.C:38-179.  oseq: filtered codes; C: the .red
    records; cpos: where to start looking.  -> (corrected codes, adjusts [(adjpos, adjust)],
    cpos after)."""
    clen = C.shape[0]
    ids = C["readID"]
    while cpos < clen and int(ids[cpos]) < cur_id:                        # :58-61
        cpos += 1
    if cpos >= clen or int(ids[cpos]) != cur_id or (int(C["word"][cpos]) >> 2) & 15 != IDENT:
        raise BadInput(f"read {cur_id} has no IDENT record")              # :65, and what it leaves open
    cpos += 1
    fseq: list[int] = []
    fadj: list[tuple[int, int]] = []
    adj_val = 0
    n = oseq.shape[0]
    i = 0
    while i < n:                                                          # :76
        if cpos == clen or int(ids[cpos]) != cur_id:                      # :79-84
            fseq.extend(int(v) for v in oseq[i:])
            break
        w = int(C["word"][cpos])
        typ, pos = (w >> 2) & 15, w >> 6
        if i < pos:                                                       # :87-90
            fseq.extend(int(v) for v in oseq[i:pos if pos < n else n])
            i = pos if pos < n else n
            continue
        if i != pos and i != pos + 1:                                     # :95-96
            raise BadInput(f"read {cur_id}: at base {i}, a correction of base {pos}")
        if changes is not None:
            changes[typ] += 1
        if typ == DELETE:                                                 # :102-107
            adj_val -= 1
            fadj.append((i + 1, adj_val))
        elif A_SUBST <= typ <= T_SUBST:                                   # :109-112
            fseq.append(typ - A_SUBST)
        elif A_INSERT <= typ <= T_INSERT:                                 # :114-164
            if i != pos + 1:
                fseq.append(int(oseq[i]))
                i += 1
                _bump(branches, "insert_copy")
            else:
                _bump(branches, "insert_after_subst")
            fseq.append(typ - A_INSERT)
            adj_val += 1
            fadj.append((i + 1, adj_val))
            i -= 1
        else:
            raise BadInput(f"read {cur_id}: a correction of type {typ}")   # :166-168 skips the base
        cpos += 1
        i += 1
    return np.array(fseq, dtype=np.uint8), fadj, cpos


def make_rev_adjust(fadj, frag_len: int, branches=None):
    """Make_Rev_Adjust, correctOverlaps-Redo_Olaps.C:173-230."""
    ct = len(fadj)
    if ct == 0:
        return []
    _bump(branches, "rev_adjust")
    radj = []
    prev = 0
    for i in range(ct - 1, 0, -1):
        if fadj[i][1] == fadj[i - 1][1] + 1:
            radj.append((2 + frag_len - fadj[i][0], prev + 1))
        elif fadj[i][1] == fadj[i - 1][1] - 1:
            radj.append((3 + frag_len - fadj[i][0], prev - 1))
        else:
            raise AssertionError("Bad adjustment value")
        prev = radj[-1][1]
    if fadj[0][1] == 1:
        radj.append((2 + frag_len - fadj[0][0], prev + 1))
    elif fadj[0][1] == -1:
        radj.append((3 + frag_len - fadj[0][0], prev - 1))
    else:
        raise AssertionError("Bad adjustment value")
    return radj


def hang_adjust(hang: int, adjust) -> int:
    """Hang_Adjust, correctOverlaps-Redo_Olaps.C:238-257."""
    assert hang >= 0
    delta = 0
    for adjpos, adj in adjust:
        if hang < adjpos:
            break
        delta = adj
    return hang + delta


# ------------------------------------------------------------------------- the aligner

def prefix_edit_dist(A, T, limit: int, ML, stats=None):
    """Prefix_Edit_Dist, correctOverlaps-Prefix_Edit_Distance.C:165-312.
    -> (errors, a_end, t_end, match_to_end, delta)."""
    m, n = A.shape[0], T.shape[0]
    shorter = min(m, n)
    ne = np.nonzero(A[:shorter] != T[:shorter])[0]
    row0 = int(ne[0]) if ne.size else shorter
    if row0 == shorter:                                                   # :196-201
        return 0, row0, row0, True, []
    Ap = np.concatenate([A, np.full(40, 254, np.uint8)])
    Tp = np.concatenate([T, np.full(40, 255, np.uint8)])
    R = FR._Rows()
    R.push(0, np.array([row0], dtype=np.int64), 0, 0)
    left = right = 0
    best_d = longest = 0
    max_score = 0.0
    ms_len = ms_d = 0
    used = 1
    for e in range(1, limit + 1):
        left = max(left - 1, -e)
        right = min(right + 1, e)
        ds = np.arange(left, right + 1)
        P = np.full(right - left + 3, -2, dtype=np.int64)     # row e-1 on [left-1, right+1]
        lo, hi, b = R.lo[e - 1], R.hi[e - 1], R.base[e - 1]
        P[lo - (left - 1):hi - (left - 1) + 1] = R.val[e - 1][lo - b:hi - b + 1]
        row = np.maximum(np.maximum(1 + P[1:-1], P[:-2]), P[2:] + 1)
        FR._slide(Ap, Tp, row, ds)
        if stats is not None:
            stats["rows"] = stats.get("rows", 0) + 1
            used += right - left + 1
            stats["max_width"] = max(stats.get("max_width", 0), right - left + 1)
            stats["log_used"] = max(stats.get("log_used", 0), used)
        end = np.nonzero((row == m) | (row + ds == n))[0]
        if end.size:                                                      # :236-254
            k = int(end[0])
            d, r = int(ds[k]), int(row[k])
            if r == m and 1 + R.get(e - 1, d + 1) == r and d < right:
                d += 1
            R.push(left, row, left, right)
            return e, r, r + d, True, FR.compute_delta(R, e, d, r)
        lim = int(ML[e])
        g = lambda d: int(row[d - ds[0]])
        while left <= right and left < 0 and g(left) < lim:                # :257-275
            left += 1
        if left >= 0:
            while left <= right and g(left) + left < lim:
                left += 1
        if left > right:
            break
        while right > 0 and g(right) + right < lim:
            right -= 1
        if right <= 0:
            while g(right) < lim:
                right -= 1
        assert left <= right
        R.push(int(ds[0]), row, left, right)
        seg = row[left - ds[0]:right - ds[0] + 1]
        k = int(np.argmax(seg))
        if int(seg[k]) > longest:                                         # :279-284
            best_d, longest = left + k, int(seg[k])
        score = int(longest * BRANCH_PT_MATCH_VALUE - e)                  # :286, int32: truncated
        if score > max_score:                                             # :292, the one test
            max_score = float(score)
            ms_len, ms_d = longest, best_d
    return limit + 1, ms_len, ms_len + ms_d, False, []                    # :303-311, deltaLen 0


# ----------------------------------------------------------------------------- the job

def correct_overlaps(records, reads: dict, red: np.ndarray, bgn: int, end: int, erate: float,
                     branches=None, stats=None):
    """Correct_Frags and Redo_Olaps -> (evalues in input order, counters dict).  reads: id ->
    bytes; red: the .red records.  The overlaps are taken one by one, each with its own look-up
    of its B read's corrections: with records ascending by read that is what the reference's
    single pass over the sorted overlaps finds."""
    red = np.ascontiguousarray(red, dtype=RED_DTYPE)
    if red.shape[0] > 1 and (np.diff(red["readID"].astype(np.int64)) < 0).any():
        raise BadInput("corrections are not ascending by read")
    changes = [0] * 16
    cor: dict = {}
    nbases = 0
    cpos = 0
    for rid in range(bgn, end + 1):                                       # Correct_Frags :265-322
        seq, fadj, cpos = correct_read(rid, filter_read(reads[rid]), red, cpos, changes, branches)
        cor[rid] = (seq, fadj)
        nbases += seq.shape[0] + 1
    c = {k: 0 for k in COUNTERS}
    c["corrected_bases"] = nbases
    c["substitutions"] = sum(changes[A_SUBST:T_SUBST + 1])
    c["deletions"] = changes[DELETE]
    c["insertions"] = sum(changes[A_INSERT:T_INSERT + 1])
    bcor: dict = {}

    def b_read(rid):
        if rid not in bcor:
            if rid not in reads:
                raise BadInput(f"read {rid} is not loaded")
            at = int(np.searchsorted(red["readID"], rid, side="left"))
            seq, fadj, _ = correct_read(rid, filter_read(reads[rid]), red, at, None, branches)
            bcor[rid] = (seq, fadj, (3 - seq)[::-1], make_rev_adjust(fadj, seq.shape[0], branches))
        return bcor[rid]

    maxlen = max([len(r) for r in reads.values()] + [1]) + 64
    ML = match_limit(erate, error_bound(2 * maxlen, erate) + 2)
    out = np.zeros(len(records), dtype=np.uint16)
    for k, rec in enumerate(records):                                     # Redo_Olaps :365-524
        a, b, a_hang, _b_hang, flipped = unpack_olap(rec)
        if not bgn <= a <= end:
            raise BadInput(f"a_iid {a} outside {bgn}-{end}")
        aseq, aadj = cor[a]
        fseq, fadj, rseq, radj = b_read(b)
        a_part = aseq
        if a_hang > 0:                                                    # :375-381
            ha = hang_adjust(a_hang, aadj)
            _probe(branches, "a", a_hang, aadj)
            if ha > aseq.shape[0]:
                raise BadInput("adjusted hang past the end of A")
            if ha != a_hang:
                _bump(branches, "hang_a")
            a_part = aseq[ha:]
        b_part = rseq if flipped else fseq
        c["olaps_rev" if flipped else "olaps_fwd"] += 1
        rha = False
        if a_hang < 0:                                                    # :398-404
            ha = hang_adjust(-a_hang, radj if flipped else fadj)
            _probe(branches, "b_rev" if flipped else "b_fwd", -a_hang, radj if flipped else fadj)
            if ha > b_part.shape[0]:
                raise BadInput("adjusted hang past the end of B")
            if ha != -a_hang:
                _bump(branches, "hang_b_rev" if flipped else "hang_b_fwd")
            b_part = b_part[ha:]
            rha = True
        olap_len = min(a_part.shape[0], b_part.shape[0])
        if stats is not None:
            stats["bases"] = stats.get("bases", 0) + olap_len
        errors, a_end, b_end, to_end, delta = prefix_edit_dist(
            a_part, b_part, error_bound(olap_len, erate), ML, stats)
        if delta and delta[0] == 1 and a_hang > 0:                        # :431-448
            stop = min(len(delta), a_hang)
            i = 0
            while i < stop and delta[i] == 1:
                i += 1
            _bump(branches, "trim_a_stop" if i == stop else "trim_a_short")
            if i == stop and len(delta) < a_hang:
                _bump(branches, "trim_a_all")
            a_end -= i
            errors -= i
        elif delta and delta[0] == -1 and a_hang < 0:                     # :450-468
            stop = min(len(delta), -a_hang)
            i = 0
            while i < stop and delta[i] == -1:
                i += 1
            _bump(branches, "trim_b_stop" if i == stop else "trim_b_short")
            if i == stop and len(delta) < -a_hang:
                _bump(branches, "trim_b_all")
            b_end -= i
            errors -= i
        c["total"] += 1
        olen = min(a_end, b_end)                                          # :474
        if not to_end and olen <= 0:
            c["failed_both"] += 1
            _bump(branches, "fail_both")
        if not to_end:
            c["failed_end"] += 1
            _bump(branches, "fail_end")
        if olen <= 0:
            c["failed_length"] += 1
            _bump(branches, "fail_length")
        if not to_end or olen <= 0:                                       # :485-516
            c["failed_either"] += 1
            c["rha_fail"] += rha
            out[k] = evalue_of(rec)
            continue
        c["rha_pass"] += rha
        out[k] = encode_evalue(errors / olen)                             # :521
    return out, c


def oea_bytes(bgn: int, end: int, evalues) -> bytes:
    """correctOverlaps.C:203-215."""
    ev = np.ascontiguousarray(evalues, dtype="<u2")
    return struct.pack("<IIQ", bgn, end, ev.shape[0]) + ev.tobytes()


# ----------------------------------------------------------------------------- the fixtures

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("a", "b", "c", "d", "e")
_golden: dict = {}


def golden(name: str) -> dict:
    """tests/golden/co_<name>.npz (tools/make_co_golden.py): rs, the store's records of the
    range in store order, the .red records, the reference's .oea bytes, its counters (the nine
    and the four of the "Corrected" line), bgn, end, erate."""
    if name not in _golden:
        from canu_amd.overlap_in_core import RECORD_DTYPE
        from canu_amd.synth import ReadSet
        z = np.load(os.path.join(GOLDEN, f"co_{name}.npz"))
        rs = ReadSet(bases=z["bases"], offsets=z["offsets"], lengths=z["lengths"], first_iid=1)
        inp = np.zeros(z["in_a"].shape[0], dtype=RECORD_DTYPE)
        for f in RECORD_DTYPE.names:
            inp[f] = z["in_" + f]
        red = np.frombuffer(z["red"].tobytes(), dtype=RED_DTYPE)
        for arr in (inp, rs.bases, rs.offsets, rs.lengths):
            arr.setflags(write=False)
        cnt = [int(v) for v in z["counters"]]
        _golden[name] = {
            "rs": rs, "records": inp, "red": red, "oea": z["oea"].tobytes(),
            "counters": dict(zip(COUNTERS + CORRECTED, cnt[:13])),
            "bgn": cnt[13], "end": cnt[14],
            "erate": float(z["args"].tobytes().decode().split()[1])}
    return _golden[name]
