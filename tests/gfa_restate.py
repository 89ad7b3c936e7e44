"""A restatement of canu's alignGFA (src/gfa/alignGFA.C, gfa.C, bed.C and the edlib calls they
make) in Python, for the tests of canu_amd.align_gfa.

The three modes are restated literally -- the same steps in the same order, the same doubles --
with edlib's results in the closed forms of tests/fs_restate.py: `locate` for EDLIB_MODE_HW
(distance, first best end, longest start), the bottom-right cell for EDLIB_MODE_NW, `path` for
EDLIB_TASK_PATH.  Each mode returns the output file, stderr (plain or -V) and fills a branch
log; tests/golden/gfa_*.npz pin all of it to the reference binary (tests/test_gfa_cpu.py).

Where the reference asserts or reads outside a sequence, `Refused` is raised.
"""
from __future__ import annotations

import math
import os
import re
import struct

import numpy as np

import fs_restate as FS

END_BASES = 50000                                     # alignGFA.C:480
MIN_OLAP = 100                                        # alignGFA.C:725
U32MAX = 0xFFFFFFFF

REQUIRED_BRANCHES = (
    # links
    "link_kept", "link_dropped", "ori_++", "ori_+-", "ori_-+", "ori_--", "circular",
    "circular_unequal", "extB_fail_extA_ok", "abgn_clamped", "bend_clamped", "query_longer",
    "cigar_I", "cigar_D", "gapped_consensus", "deleted_unreferenced", "n_fwd_vs_n_rev",
    # placements
    "rec_kept", "rec_dropped", "accept_first_round_contig_end", "extend_left", "extend_right",
    "relax_then_success", "relax_abort", "rec_reversed", "left_right", "len_49999",
    # BED to GFA
    "pair_kept", "pair_diff_contig", "pair_thin", "link_star", "olap_override", "double_H")


class Refused(ValueError):
    """What libcanu_gfa answers with GFA_ERR_BAD_INPUT."""


def new_log() -> dict:
    log = {k: 0 for k in REQUIRED_BRANCHES}
    log.update(FS.new_log())
    log.update({"alignments": 0, "rounds_max": 0})
    return log


# ------------------------------------------------------------------ sequences

_RC = bytearray(256)                                  # AS_UTL_reverseComplement.C:39-72
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _RC[_a] = _b
_RC = bytes(_RC)


def revcomp(b: bytes) -> bytes:
    """reverseComplementCopy: every byte outside ACGTacgt, N included, becomes NUL."""
    return b.translate(_RC)[::-1]


def ungap(gapped: bytes) -> bytes:
    return gapped.replace(b"-", b"")


def encode_tigstore(tigs: list, version: int = 2) -> tuple[bytes, bytes]:
    """seqDB.v<version>.tig and .dat of a store whose tig i has the gapped consensus tigs[i];
    None is an entry marked deleted."""
    n = len(tigs)
    dat = bytearray()
    tig = bytearray(struct.pack("<IIIII", FS.MASR_MAGIC, 1, n, 0, n))
    for t, g in enumerate(tigs):
        if g is None:
            tig += FS.TIG_RECORD.pack(t, 0.0, 0.0, 0, 0, 0, 0, 0) + struct.pack("<Q", 1 << 13)
            continue
        rec = FS.TIG_RECORD.pack(t, 0.0, 0.0, 0, len(ungap(g)), len(g), 0, 0)
        tig += rec + struct.pack("<Q", (version << 14) | (len(dat) << 24))
        dat += b"TIGR" + rec + g + b"!" * len(g)
    return bytes(tig), bytes(dat)


def decode_tigstore(tig: bytes, dat: bytes, log: dict | None = None) -> list:
    """-> the ungapped bases of every tig (b"" for a deleted one), as `sequences` loads them."""
    magic, version, total, _, n = struct.unpack_from("<IIIII", tig, 0)
    if magic != FS.MASR_MAGIC or version != 1 or len(tig) != 20 + n * FS.STORE_ENTRY_BYTES:
        raise ValueError("not a tig index")
    out = []
    for k in range(n):
        base = 20 + k * FS.STORE_ENTRY_BYTES
        (word,) = struct.unpack_from("<Q", tig, base + FS.TIG_RECORD.size)
        if (word >> 13) & 1 or ((word >> 14) & 1023) == 0:
            out.append(b"")
            continue
        off = word >> 24
        if dat[off:off + 4] != b"TIGR":
            raise ValueError(f"tig {k}: no record at {off}")
        tid, _, _, _, _, glen, _, _ = FS.TIG_RECORD.unpack_from(dat, off + 4)
        g = bytes(dat[off + 4 + FS.TIG_RECORD.size:off + 4 + FS.TIG_RECORD.size + glen])
        if len(g) != glen or tid != k:
            raise ValueError(f"tig {k}: short record")
        out.append(ungap(g))
        if log is not None and b"-" in g:
            log["gapped_consensus"] += 1
    return out


def _seq(seqs: list, tid: int) -> bytes:
    if tid >= len(seqs):
        raise Refused(f"tig {tid} is outside the {len(seqs)} tigs loaded")
    if len(seqs[tid]) == 0:
        raise Refused(f"tig {tid} has no sequence")
    return seqs[tid]


# ------------------------------------------------------------------ files

def strtoll(s: str) -> int:
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def name_to_id(name: str) -> int:
    """nameToCanuID (gfa.C:59-70, bed.C:34-55)."""
    if name[:3] in ("tig", "utg", "ctg"):
        return strtoll(name[3:]) & U32MAX
    return U32MAX


def _words(line: str) -> list:
    return line.split()                               # splitToWords: spaces and tabs


def parse_gfa(text: str):
    """gfaFile::loadFile -> (header, sequences, links)."""
    header, seqs, links = None, [], []
    for line in text.split("\n"):
        if line == "":
            continue
        if len(line) < 2 or line[1] != "\t":
            raise Refused(f"misformed line '{line}'")
        if line[0] == "H":
            header = line[2:]
        elif line[0] == "S":
            w = _words(line)
            if len(w) < 4:
                raise Refused(f"S line with {len(w)} fields")
            seqs.append({"name": w[1], "seq": w[2], "features": w[3], "id": name_to_id(w[1])})
        elif line[0] == "L":
            w = _words(line)
            if len(w) < 6:
                raise Refused(f"L line with {len(w)} fields")
            links.append({"Aname": w[1], "Afwd": w[2][0] == "+", "Bname": w[3],
                          "Bfwd": w[4][0] == "+", "cigar": w[5], "Aid": name_to_id(w[1]),
                          "Bid": name_to_id(w[3])})
        else:
            raise Refused(f"unrecognized line '{line}'")
    return header, seqs, links


def parse_bed(text: str) -> list:
    recs = []
    for line in text.split("\n"):
        if line == "":
            continue
        w = _words(line)
        if len(w) < 6:
            raise Refused(f"BED line with {len(w)} fields")
        recs.append({"Aname": w[0], "bgn": strtoll(w[1]), "end": strtoll(w[2]), "Bname": w[3],
                     "score": strtoll(w[4]) & U32MAX, "Bfwd": w[5][0] == "+",
                     "Aid": name_to_id(w[0]), "Bid": name_to_id(w[3])})
    return recs


def alignment_length(cigar: str, err: list) -> tuple[int, int, int]:
    """gfaLink::alignmentLength (gfa.C:224-285) -> (queryLen, refceLen, alignLen)."""
    q = r = a = 0
    if cigar is None or cigar.startswith("*"):
        return q, r, a
    pos = 0
    while True:
        m = re.match(r"\s*[+-]?\d+", cigar[pos:])
        val = int(m.group(0)) if m else 0
        pos += m.end() if m else 0
        code = cigar[pos:pos + 1]
        pos += 1
        if code in ("M", "=", "X"):
            r += val; q += val; a += val
        elif code == "I":
            q += val; a += val
        elif code == "D":
            r += val; a += val
        elif code == "N":
            r += val
            err.append(f"warning - unsupported CIGAR code '{code}' in '{cigar}'\n")
        elif code in ("S", "H", "P"):
            err.append(f"warning - unsupported CIGAR code '{code}' in '{cigar}'\n")
        else:
            err.append(f"unknown CIGAR code '{code}' in '{cigar}'\n")
        if pos >= len(cigar):
            break
    return q, r, a


def cigar_of(ops: bytes) -> str:
    """edlibAlignmentToCigar, EDLIB_CIGAR_STANDARD."""
    out = []
    last, n = None, 0
    for op in ops:
        ch = "MIDM"[op]
        if ch != last and last is not None:
            out.append(f"{n}{last}")
            n = 0
        last = ch
        n += 1
    if last is not None:
        out.append(f"{n}{last}")
    return "".join(out)


def cigar_runs(cigar: str) -> list:
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cigar)]


# ------------------------------------------------------------------ checkLink

def _hw(q: bytes, t: bytes, k: int, log: dict, need_start: bool = True):
    """EDLIB_MODE_HW -> (distance, start, end) or None.  Where the caller reads the end alone
    (extend B), the pass that finds the start is left out, and start is None."""
    if len(q) == 0 or len(t) == 0:
        raise Refused("an empty query or target")
    log["alignments"] += 1
    if need_start:
        return FS.locate(q, t, k, log)
    bottom, _, _, _ = FS.myers(q, t, 0)
    log["cells"] += len(q) * len(t)
    best = min(bottom)
    return None if best > k else (best, None, bottom.index(best))


def check_link(link: dict, seqs: list, log: dict, err: list | None):
    """checkLink (alignGFA.C:156-317): sets link['cigar'] (None: no alignment) and returns a
    dict of every intermediate value.  err: the -V lines, or None.  link['lengths'], where
    given, stands for what alignmentLength reads from the CIGAR."""
    A, B = _seq(seqs, link["Aid"]), _seq(seqs, link["Bid"])
    Alen, Blen = len(A), len(B)
    warn = []
    if "lengths" in link:                             # as the C API takes them: three numbers
        AalignLen, BalignLen, alignLen = link["lengths"]
    else:
        AalignLen, BalignLen, alignLen = alignment_length(link["cigar"], warn)
    if err is not None or warn:
        (err if err is not None else link.setdefault("warn", [])).extend(warn)
    link["cigar"] = None
    if not link["Afwd"]:
        A = revcomp(A)
    if not link["Bfwd"]:
        B = revcomp(B)
    a_s, b_s = "+" if link["Afwd"] else "-", "+" if link["Bfwd"] else "-"
    log["ori_" + a_s + b_s] += 1
    Aid, Bid = link["Aid"], link["Bid"]
    R = {"a_len": Alen, "b_len": Blen}

    Abgn, Aend = max(Alen - AalignLen, 0), Alen
    Bbgn, Bend = 0, min(Blen, int(1.10 * BalignLen))
    maxEdit = int(math.ceil(alignLen * 0.12))
    if Alen - AalignLen < 0:
        log["abgn_clamped"] += 1
    if int(1.10 * BalignLen) > Blen:
        log["bend_clamped"] += 1
    R.update(max_edit=maxEdit, abgn_b=Abgn, bend_b=Bend)
    if err is not None:
        err.append("LINK tig%08u %c %17s    tig%08u %c %17s   Aalign %6u Balign %6u align %6u\n"
                   % (Aid, a_s, "", Bid, b_s, "", AalignLen, BalignLen, alignLen))
        err.append("TEST tig%08u %c %8d-%-8d    tig%08u %c %8d-%-8d  maxEdit=%6d  (extend B)"
                   % (Aid, a_s, Abgn, Aend, Bid, b_s, Bbgn, Bend, maxEdit))
    res = _hw(A[Abgn:Aend], B[Bbgn:Bend], maxEdit, log, need_start=False)
    extB = res is not None
    if res is not None:
        Bend = Bbgn + res[2] + 1
    if err is not None:
        err.append("\n" if res is not None else " - FAILED\n")
    R.update(dist_b=res[0] if res else -1, bend=Bend)

    Abgn = max(Alen - int(1.10 * AalignLen), 0)
    if Alen - int(1.10 * AalignLen) < 0:
        log["abgn_clamped"] += 1
    if err is not None:
        err.append("     tig%08u %c %8d-%-8d    tig%08u %c %8d-%-8d  maxEdit=%6d  (extend A)"
                   % (Aid, a_s, Abgn, Aend, Bid, b_s, Bbgn, Bend, maxEdit))
    if Bend - Bbgn > Aend - Abgn:
        log["query_longer"] += 1
    R.update(abgn_a=Abgn)
    res = _hw(B[Bbgn:Bend], A[Abgn:Aend], maxEdit, log)
    if res is not None:
        Abgn += res[1]
        if not extB:
            log["extB_fail_extA_ok"] += 1
    if err is not None:
        err.append("\n" if res is not None else " - FAILED\n")
    R.update(dist_a=res[0] if res else -1, abgn=Abgn)

    if err is not None:
        err.append("     tig%08u %c %8d-%-8d    tig%08u %c %8d-%-8d  maxEdit=%6d  (final)"
                   % (Aid, a_s, Abgn, Aend, Bid, b_s, Bbgn, Bend, maxEdit))
    q, t = A[Abgn:Aend], B[Bbgn:Bend]
    if len(q) == 0 or len(t) == 0:
        raise Refused("an empty query or target")
    log["alignments"] += 1
    bottom, _, _, _ = FS.myers(q, t, 1)
    log["cells"] += len(q) * len(t)
    dist = bottom[-1]
    editDist, success = 0, False
    R.update(dist_f=-1, align_len=0, leaf=0, split=0)
    if dist <= 2 * maxEdit:
        leaf0, split0 = log["leaf"], log["split"]
        ops = FS.path(q, t, dist, log)
        editDist, alignLen, success = dist, len(ops), True
        link["cigar"] = cigar_of(ops)
        if "I" in link["cigar"]:
            log["cigar_I"] += 1
        if "D" in link["cigar"]:
            log["cigar_D"] += 1
        if (b"N" in q and b"\0" in t) or (b"\0" in q and b"N" in t):
            log["n_fwd_vs_n_rev"] += 1
        R.update(dist_f=dist, align_len=alignLen, leaf=log["leaf"] - leaf0,
                 split=log["split"] - split0)
    if err is not None:
        err.append("\n" if success else " - FAILED\n")
        ratio = editDist / alignLen if alignLen else float("nan")
        err.append("     tig%08u %c %8d-%-8d    tig%08u %c %8d-%-8d   %.4f\n"
                   % (Aid, a_s, Abgn, Aend, Bid, b_s, Bbgn, Bend, ratio))
        err.append("\n")
    log["link_kept" if success else "link_dropped"] += 1
    R.update(success=success, cigar=link["cigar"])
    return R


def _save_gfa(header, seqs: list, links: list) -> str:
    out = ["H\t%s\n" % header]
    out += ["S\t%s\t%s\tLN:i:%u\n" % (s["name"], s["seq"], s["length"]) for s in seqs]
    out += ["L\t%s\t%c\t%s\t%c\t%s\n" % (l["Aname"], "+" if l["Afwd"] else "-", l["Bname"],
                                        "+" if l["Bfwd"] else "-",
                                        "*" if l["cigar"] is None else l["cigar"])
            for l in links if l is not None]
    return "".join(out)


def process_gfa(seqs: list, text: str, names: dict, verbose: bool, log: dict | None = None):
    """processGFA at -t 1 -> (output file, stderr, per-link results)."""
    log = new_log() if log is None else log
    err = ["-- Reading GFA '%s'.\n" % names["in"]]
    header, S, L = parse_gfa(text)
    err.append("gfa:  Loaded %d sequences and %d links.\n" % (len(S), len(L)))
    err.append("-- Loading sequences from tigStore '%s' version %u.\n" % (names["T"], names["Tv"]))
    err.append("-- Resetting sequence lengths.\n")
    for s in S:
        if s["id"] >= len(seqs):
            raise Refused(f"sequence {s['name']} is outside the store")
        s["length"] = len(seqs[s["id"]])
    err.append("-- Aligning %u links using %u threads.\n" % (len(L), 1))
    pc = fc = pn = fn = 0
    results = []
    referenced = set()
    for ii, link in enumerate(L):
        referenced |= {link["Aid"], link["Bid"]}
        circ = link["Aid"] == link["Bid"]
        if circ:
            log["circular"] += 1
            if verbose:
                err.append("Processing circular link for tig %u\n" % link["Aid"])
            if link["Afwd"] != link["Bfwd"]:
                log["circular_unequal"] += 1
                err.append("WARNING: %s %c %s %c -- circular to the same end!?\n"
                           % (link["Aname"], "+" if link["Afwd"] else "-", link["Bname"],
                              "+" if link["Bfwd"] else "-"))
        elif verbose:
            err.append("Processing link between tig %u %s and tig %u %s\n"
                       % (link["Aid"], "-->" if link["Afwd"] else "<--", link["Bid"],
                          "-->" if link["Bfwd"] else "<--"))
        v = [] if verbose else None
        R = check_link(link, seqs, log, v)
        err += link.pop("warn", [])
        if verbose:
            err += v
        results.append(R)
        if circ:
            pc, fc = pc + R["success"], fc + (not R["success"])
        else:
            pn, fn = pn + R["success"], fn + (not R["success"])
        if link["cigar"] is None:
            if verbose:
                err.append("  Failed to find alignment.\n")
            L[ii] = None
    if any(len(s) == 0 and i not in referenced for i, s in enumerate(seqs)):
        log["deleted_unreferenced"] += 1
    err.append("-- Writing GFA '%s'.\n" % names["out"])
    out = _save_gfa(header, S, L)
    err.append("-- Cleaning up.\n")
    err.append("-- Aligned %6u ciruclar tigs, failed %6u\n" % (pc, fc))
    err.append("-- Aligned %6u   linear tigs, failed %6u\n" % (pn, fn))
    err.append("Bye.\n")
    return out, "".join(err), results


# ------------------------------------------------------------------ checkRecord

CALLS = ("ALL", "LEFT", "RIGHT")


def check_record_align(label: str, Aname: str, A: bytes, Abgn: int, Aend: int, Bname: str,
                       B: bytes, log: dict, err: list | None, tries: list):
    """checkRecord_align (alignGFA.C:324-452) -> (success, Abgn, Aend)."""
    Alen, Blen = len(A), len(B)
    maxEdit = int(math.ceil(Blen * 0.03))
    step = int(math.ceil(Blen * 0.15))
    Aend = min(Aend + 2 * step, Alen)
    Abgn = max(Aend - Blen - 2 * step, 0)
    rounds, relaxed = 0, False
    while True:
        rounds += 1
        log["rounds_max"] = max(log["rounds_max"], rounds)
        if err is not None:
            err.append("ALIGN %5s utg %s len=%7d to ctg %s %9d-%9d len=%9d"
                       % (label, Bname, Blen, Aname, Abgn, Aend, Alen))
        res = _hw(B, A[Abgn:Aend], maxEdit, log)
        T = {"call": CALLS.index(label), "b_len": Blen, "abgn": Abgn, "aend": Aend,
             "max_edit": maxEdit, "dist": -1, "nbgn": 0, "nend": 0}
        tries.append(T)
        if res is not None:
            editDist = res[0]
            nAbgn, nAend = Abgn + res[1], Abgn + res[2] + 1
            alignLen = ((nAend - nAbgn) + Blen + editDist) // 2
            score = 1000 - int(1000.0 * editDist / alignLen)
            T.update(dist=editDist, nbgn=nAbgn, nend=nAend)
            if err is not None:
                err.append(" - POSITION from %9d-%-9d to %9d-%-9d score %5d/%9d = %4d%s%s\n"
                           % (Abgn, Aend, nAbgn, nAend, editDist, alignLen, score, "", ""))
            if (Abgn < nAbgn or Abgn == 0) and (nAend < Aend or Aend == Alen):
                if rounds == 1 and ((Abgn == 0 and nAbgn == 0) or (Aend == Alen and nAend == Alen)):
                    log["accept_first_round_contig_end"] += 1
                if relaxed:
                    log["relax_then_success"] += 1
                T["outcome"] = 0
                return True, nAbgn, nAend
            T["outcome"] = 1
            if Abgn == nAbgn:
                log["extend_left"] += 1
                Abgn = max(Abgn - step, 0)
            if Aend == nAend:
                log["extend_right"] += 1
                Aend = min(Aend + step, Alen)
            continue
        if (Aend - Abgn < 4 * Blen) and (maxEdit < Blen * 0.25):
            if err is not None:
                err.append(" - FAILED, RELAX\n")
            T["outcome"] = 2
            relaxed = True
            Abgn = max(Abgn - step, 0)
            Aend = min(Aend + step, Alen)
            maxEdit = int(maxEdit * 1.2)
            continue
        if err is not None:
            err.append(" - ABORT, ABORT, ABORT!\n")
        T["outcome"] = 3
        if relaxed:
            log["relax_abort"] += 1
        return False, Abgn, Aend


def check_record(rec: dict, ctgs: list, utgs: list, log: dict, err: list | None):
    """checkRecord (alignGFA.C:456-537): updates rec on success; -> (success, tries)."""
    A, B = _seq(ctgs, rec["Aid"]), _seq(utgs, rec["Bid"])
    Abgn, Aend, Alen, Blen = rec["bgn"], rec["end"], len(A), len(B)
    if Abgn < 0 or Aend < Abgn or Aend > Alen:
        raise Refused(f"{Abgn}-{Aend} is outside contig {rec['Aid']} of {Alen} bases")
    if not rec["Bfwd"]:
        B = revcomp(B)
        log["rec_reversed"] += 1
    tries: list = []
    if Blen < END_BASES:
        if Blen == END_BASES - 1:
            log["len_49999"] += 1
        ok, Abgn, Aend = check_record_align("ALL", rec["Aname"], A, Abgn, Aend, rec["Bname"], B,
                                            log, err, tries)
    else:
        log["left_right"] += 1
        okL, AbgnL, _ = check_record_align("LEFT", rec["Aname"], A, Abgn, Abgn + END_BASES,
                                           rec["Bname"], B[:END_BASES], log, err, tries)
        okR, _, AendR = check_record_align("RIGHT", rec["Aname"], A, Aend - END_BASES, Aend,
                                           rec["Bname"], B[Blen - END_BASES:], log, err, tries)
        ok, Abgn, Aend = okL and okR, AbgnL, AendR
    if ok:
        rec["bgn"], rec["end"], rec["score"] = Abgn, Aend, 0
    log["rec_kept" if ok else "rec_dropped"] += 1
    return ok, tries


def _save_bed(recs: list) -> str:
    return "".join("%s\t%d\t%d\t%s\t%u\t%c\n" % (r["Aname"], r["bgn"], r["end"], r["Bname"],
                                                 r["score"], "+" if r["Bfwd"] else "-")
                   for r in recs if r is not None)


def process_bed(utgs: list, ctgs: list, text: str, names: dict, verbose: bool,
                log: dict | None = None):
    """processBED at -t 1 -> (output file, stderr, per-record (success, bgn, end, tries))."""
    log = new_log() if log is None else log
    err = ["-- Reading BED '%s'.\n" % names["in"]]
    recs = parse_bed(text)
    err.append("bed:  Loaded %d records.\n" % len(recs))
    err.append("-- Loading sequences from tigStore '%s' version %u.\n" % (names["T"], names["Tv"]))
    err.append("-- Loading sequences from tigStore '%s' version %u.\n" % (names["C"], names["Cv"]))
    err.append("-- Aligning %u records using %u threads.\n" % (len(recs), 1))
    npass = nfail = 0
    results = []
    for ii, rec in enumerate(recs):
        v = [] if verbose else None
        ok, tries = check_record(rec, ctgs, utgs, log, v)
        if verbose:
            err += v
        results.append((ok, rec["bgn"], rec["end"], tries))
        if ok:
            npass += 1
        else:
            recs[ii] = None
            nfail += 1
    err.append("-- Writing BED '%s'.\n" % names["out"])
    out = _save_bed(recs)
    err.append("-- Cleaning up.\n")
    err.append("-- Aligned %6u unitigs to contigs, failed %6u\n" % (npass, nfail))
    err.append("Bye.\n")
    return out, "".join(err), results


# ------------------------------------------------------------------ BED to GFA

def bed_pairs(recs: list, log: dict | None = None) -> list:
    """The (ii, jj, olapLen) processBEDtoGFA aligns (alignGFA.C:751-775), in -t 1 order."""
    pairs = []
    for ii in range(len(recs)):
        for jj in range(ii + 1, len(recs)):
            a, b = recs[ii], recs[jj]
            if a["Aid"] != b["Aid"]:
                if log is not None:
                    log["pair_diff_contig"] += 1
                continue
            if a["end"] < b["bgn"] + MIN_OLAP or b["end"] < a["bgn"] + MIN_OLAP:
                if log is not None:
                    log["pair_thin"] += 1
                continue
            olap = 0
            first = False
            if a["bgn"] < b["end"]:
                olap = a["end"] - b["bgn"]
                first = True
            if b["bgn"] < a["end"]:
                if first and log is not None:
                    log["olap_override"] += 1
                olap = b["end"] - a["bgn"]
            if olap <= 0:
                raise Refused("olapLen <= 0")
            if log is not None:
                log["pair_kept"] += 1
            pairs.append((ii, jj, olap))
    return pairs


def process_bed_to_gfa(utgs: list, text: str, names: dict, verbose: bool, log: dict | None = None):
    """processBEDtoGFA at -t 1 -> (output file, stderr, per-link results)."""
    log = new_log() if log is None else log
    err = ["-- Loading sequences from tigStore '%s' version %u.\n" % (names["T"], names["Tv"])]
    err.append("-- Reading BED '%s'.\n" % names["in"])
    recs = parse_bed(text)
    err.append("bed:  Loaded %d records.\n" % len(recs))
    err.append("-- Aligning %u records using %u threads.\n" % (len(recs), 1))
    links, results = [], []
    used = [0] * len(utgs)
    for ii, jj, olap in bed_pairs(recs, log):
        a, b = recs[ii], recs[jj]
        link = {"Aname": a["Bname"], "Afwd": True, "Bname": b["Bname"], "Bfwd": True,
                "cigar": "%dM" % olap, "Aid": name_to_id(a["Bname"]), "Bid": name_to_id(b["Bname"])}
        v = [] if verbose else None
        results.append(check_link(link, utgs, log, v))
        if verbose:
            err += v
        if link["cigar"] is None:
            log["link_star"] += 1
        links.append(link)
        used[a["Bid"]] += 1
        used[b["Bid"]] += 1
    S = [{"name": "utg%08u" % i, "seq": "*", "length": len(utgs[i])}
         for i in range(len(utgs)) if used[i] > 0]
    log["double_H"] += 1
    out = _save_gfa("H\tVN:Z:bogart/edges", S, links)
    err.append("Bye.\n")
    return out, "".join(err), results


# ------------------------------------------------------------------ the program and fixtures

def parse_args(argv: list) -> dict:
    """main() of alignGFA.C:823-925; an unknown option or a missing one raises ValueError."""
    o = {"T": None, "Tv": U32MAX, "C": None, "Cv": U32MAX, "type": "gfa", "in": None, "out": None,
         "verbose": 0, "threads": None}
    i = 0
    bad = 0
    while i < len(argv):
        a = argv[i]
        if a in ("-T", "-C"):
            o[a[1]] = argv[i + 1]
            o[a[1] + "v"] = FS.atoi(argv[i + 2]) & U32MAX
            i += 2
        elif a in ("-gfa", "-bed"):
            o["type"] = a[1:]
        elif a in ("-i", "-o"):
            o["in" if a == "-i" else "out"] = argv[i + 1]
            i += 1
        elif a == "-V":
            o["verbose"] += 1
        elif a == "-t":
            o["threads"] = FS.atoi(argv[i + 1])
            i += 1
        else:
            bad += 1
        i += 1
    if bad or o["T"] is None or o["in"] is None or o["out"] is None or o["Tv"] == 0 or \
            (o["C"] is not None and o["Cv"] == 0):
        raise ValueError("usage")
    return o


def run(argv: list, tigs_T: list, tigs_C: list | None, text: str, log: dict | None = None):
    """The program -> (output file, stderr, results)."""
    o = parse_args(argv)
    if o["type"] == "gfa":
        return process_gfa(tigs_T, text, o, o["verbose"] > 0, log)
    if o["C"] is not None:
        return process_bed(tigs_T, tigs_C, text, o, o["verbose"] > 0, log)
    return process_bed_to_gfa(tigs_T, text, o, o["verbose"] > 0, log)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("a", "b", "c", "d", "e")

_B2 = np.frombuffer(b"ACGT", dtype=np.uint8)


def pack2(seq: bytes) -> np.ndarray:
    """An all-ACGT sequence at 2 bits per base."""
    a = np.frombuffer(seq, dtype=np.uint8)
    lut = np.zeros(256, dtype=np.uint8)
    lut[list(b"ACGT")] = [0, 1, 2, 3]
    code = lut[a]
    pad = (-len(code)) % 4
    code = np.concatenate([code, np.zeros(pad, dtype=np.uint8)]).reshape(-1, 4)
    return (code[:, 0] | (code[:, 1] << 2) | (code[:, 2] << 4) | (code[:, 3] << 6)).astype(np.uint8)


def unpack2(packed: np.ndarray, n: int) -> bytes:
    p = np.asarray(packed, dtype=np.uint8)
    code = np.stack([p & 3, (p >> 2) & 3, (p >> 4) & 3, (p >> 6) & 3], axis=1).reshape(-1)[:n]
    return _B2[code].tobytes()


_golden: dict = {}


def golden(name: str) -> dict:
    """tests/golden/gfa_<name>.npz (tools/make_gfa_golden.py): the tigs of the -T and -C stores
    (None: a deleted entry; gapped where the fixture has gaps), the input text, the arguments and
    the reference's output file and stderr, plain and -V."""
    if name in _golden:
        return _golden[name]
    z = np.load(os.path.join(GOLDEN, f"gfa_{name}.npz"))
    g = {"args": z["args"].tobytes().decode().split(), "input": z["input"].tobytes().decode(),
         "out": z["out"].tobytes().decode(), "err": z["err"].tobytes().decode(),
         "out_v": z["out_v"].tobytes().decode(), "err_v": z["err_v"].tobytes().decode()}
    for which in ("T", "C"):
        if which + "_len" not in z:
            g["gapped_" + which] = None
            continue
        tigs = []
        lens, kinds = z[which + "_len"], z[which + "_kind"]
        pk, raw = z[which + "_packed"], z[which + "_raw"].tobytes()
        po = ro = 0
        for n, kind in zip(lens, kinds):
            n = int(n)
            if kind == 0:                              # deleted
                tigs.append(None)
            elif kind == 1:                            # all ACGT, packed
                nb = (n + 3) // 4
                tigs.append(unpack2(pk[po:po + nb], n))
                po += nb
            else:                                      # raw bytes (N, gaps)
                tigs.append(raw[ro:ro + n])
                ro += n
        g["gapped_" + which] = tigs
    _golden[name] = g
    return g


def store_tigs(gapped: list, log: dict | None = None) -> list:
    """The sequences alignGFA loads from a store of these (gapped) tigs: through the store's two
    files and back."""
    tig, dat = encode_tigstore(gapped)
    return decode_tigstore(tig, dat, log)


def run_golden(g: dict, verbose: bool, log: dict | None = None):
    T = store_tigs(g["gapped_T"], log)
    C = store_tigs(g["gapped_C"], log) if g["gapped_C"] is not None else None
    return run(g["args"] + (["-V"] if verbose else []), T, C, g["input"], log)
