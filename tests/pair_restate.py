"""overlapPair (src/overlapInCore/overlapPair.C:346-662) and the results of its aligner in
plain Python: the checker for libcanu_pair.so where the reference binary is absent.

The aligner is defined by what it returns, not by edlib's engine:
  infix_align(q, t, k)   EDLIB_MODE_HW / TASK_LOC: best = min over end columns j of the edit
                         distance of q against any substring of t ending at j; None if
                         best > k; end = the smallest such j; start = the smallest s with
                         ED(q, t[s..end]) == best (edlib.C:216-236: the last column at `best`
                         of a prefix pass over the reversed query and reversed t[0..end])
  global_align(q, t, k)  EDLIB_MODE_NW: the edit distance, None if > k
Bases compare as bytes: N equals only N.

Python integers are the bit vectors of Myers' recurrence (one "block" of len(q) rows);
`bottom_row_dp` is the quadratic DP the tests cross-check it with.
"""
from __future__ import annotations

import math
import os

import numpy as np

RECORD_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("w0", "<u8"), ("w1", "<u8")])

MHAP_SLOP = 500                  # overlapPair.C:64
AS_MAX_EVALUE = 4095             # ovOverlap.H:42
INT32_MAX = 2147483647
HM = (1 << 21) - 1

COUNTERS = ("nSkipped", "nPassed", "nFailed", "nFailExtA", "nFailExtB", "nFailExt", "nPartial",
            "nDovetail", "nExt5a", "nExt3a", "nExt5b", "nExt3b")

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def bottom_row(q: bytes, t: bytes, top_hin: int) -> list[int]:
    """D[len(q)][j] for every column j of t; top_hin 0 = free start in t (infix), 1 = every
    skipped base of t costs (prefix / global).  Myers 1999 with Hyyro's horizontal input."""
    m = len(q)
    mask = (1 << m) - 1
    peq: dict[int, int] = {}
    for i, c in enumerate(q):
        peq[c] = peq.get(c, 0) | (1 << i)
    pv, mv, sc = mask, 0, m
    top = 1 << (m - 1)
    out = []
    for c in t:
        eq = peq.get(c, 0)
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & mask
        ph = (mv | ~(xh | pv)) & mask
        mh = pv & xh
        if ph & top:
            sc += 1
        if mh & top:
            sc -= 1
        ph = ((ph << 1) | top_hin) & mask
        mh = (mh << 1) & mask
        pv = (mh | ~(xv | ph)) & mask
        mv = ph & xv
        out.append(sc)
    return out


def bottom_row_dp(q: bytes, t: bytes, top_hin: int) -> list[int]:
    """The same row by the quadratic recurrence."""
    m = len(q)
    col = list(range(m + 1))
    out = []
    for j, c in enumerate(t):
        new = [(j + 1) * top_hin]
        for i in range(1, m + 1):
            new.append(min(col[i] + 1, new[i - 1] + 1, col[i - 1] + (q[i - 1] != c)))
        col = new
        out.append(col[m])
    return out


def infix_align(q: bytes, t: bytes, k: int, row=bottom_row):
    """(best, start, end) with end inclusive, or None."""
    r = row(q, t, 0)
    best = min(r)
    if best > k:
        return None
    end = r.index(best)
    rr = row(q[::-1], t[:end + 1][::-1], 1)
    last = max(j for j, v in enumerate(rr) if v == best)
    return best, end - last, end


def global_align(q: bytes, t: bytes, k: int, row=bottom_row):
    d = row(q, t, 1)[-1]
    return None if d > k else d


def max_edit(a: int, b: int, erate: float) -> int:
    return int(math.ceil(max(a, b) * erate * 1.1))


def align_len(qspan: int, tspan: int, edit: int) -> int:
    return (qspan + tspan + edit) // 2


def encode_evalue(q: float) -> int:
    return int(10000.0 * q + 0.5) if q < AS_MAX_EVALUE / 10000.0 else AS_MAX_EVALUE


def unpack(rec) -> dict:
    w0, w1 = int(rec["w0"]), int(rec["w1"])
    return {"a": int(rec["a"]), "b": int(rec["b"]), "ahg5": w0 & HM, "ahg3": (w0 >> 21) & HM,
            "evalue": (w0 >> 42) & 0xfff, "flipped": (w0 >> 54) & 1, "forOBT": (w0 >> 55) & 1,
            "forDUP": (w0 >> 56) & 1, "forUTG": (w0 >> 57) & 1, "extra1": w0 >> 58,
            "bhg5": w1 & HM, "bhg3": (w1 >> 21) & HM, "rest1": w1 >> 42}


def pack(o: dict):
    w0 = (o["ahg5"] & HM) | ((o["ahg3"] & HM) << 21) | (o["evalue"] << 42) | \
         (o["flipped"] << 54) | (o["forOBT"] << 55) | (o["forDUP"] << 56) | \
         (o["forUTG"] << 57) | (o["extra1"] << 58)
    w1 = (o["bhg5"] & HM) | ((o["bhg3"] & HM) << 21) | (o["rest1"] << 42)
    return o["a"], o["b"], w0, w1


def make_record(a, b, ahg5, ahg3, bhg5, bhg3, flipped=0, evalue=0, span=0):
    o = {"a": a, "b": b, "ahg5": ahg5, "ahg3": ahg3, "bhg5": bhg5, "bhg3": bhg3,
         "flipped": int(flipped), "evalue": evalue, "forOBT": 0, "forDUP": 0, "forUTG": 0,
         "extra1": 0, "rest1": span & HM}
    return pack(o)


def swap_ids(o: dict) -> dict:
    """ovOverlap::swapIDs (ovOverlap.C:114)."""
    n = dict(o)
    n["a"], n["b"] = o["b"], o["a"]
    if not o["flipped"]:
        n["ahg5"], n["ahg3"], n["bhg5"], n["bhg3"] = o["bhg5"], o["bhg3"], o["ahg5"], o["ahg3"]
    else:
        n["ahg5"], n["ahg3"], n["bhg5"], n["bhg3"] = o["bhg3"], o["bhg5"], o["ahg3"], o["ahg5"]
    return n


class _State:
    def __init__(self):
        self.edit = INT32_MAX
        self.alen = 1


def _extend(Q, qb, qe, T, tb, te, erate, slop, st):
    """extendAlignment (:255-304); returns (ok, tb, te)."""
    tbx = max(0, tb - slop)
    tex = min(len(T), te + slop)
    k = max_edit(qe - qb, tex - tbx, erate)
    r = infix_align(Q[qb:qe], T[tbx:tex], k)
    if r is None:
        return False, tb, te
    best, s, e = r
    tb, te = tbx + s, tbx + e + 1
    st.edit = best
    st.alen = align_len(qe - qb, te - tb, best)
    return True, tb, te


def realign_one(o: dict, reads, erate: float, min_len: int, partial: bool, invert: bool,
                stats: dict) -> dict:
    """One overlap through recomputeOverlaps; `reads[iid]` are bytes; counts into stats."""
    if invert:
        o = swap_ids(o)
    o = dict(o)
    A = reads[o["a"]]
    B = reads[o["b"]]
    alen, blen = len(A), len(B)
    abgn, aend = o["ahg5"], alen - o["ahg3"]
    bbgn, bend = o["bhg5"], blen - o["bhg3"]
    st = _State()
    o["evalue"] = AS_MAX_EVALUE
    o["forOBT"] = o["forDUP"] = o["forUTG"] = 0

    def dovetail():
        return (o["ahg5"] == 0 or o["bhg5"] == 0) and (o["ahg3"] == 0 or o["bhg3"] == 0)

    def body():
        nonlocal abgn, aend, bbgn, bend, B
        if aend - abgn < min_len or bend - bbgn < min_len:
            stats["nSkipped"] += 1
            return
        if o["flipped"]:
            B = revcomp(B)
        ok, abgn, aend = _extend(B, bbgn, bend, A, abgn, aend, erate, MHAP_SLOP, st)
        if not ok:
            stats["nFailExtA"] += 1
        ok, bbgn, bend = _extend(A, abgn, aend, B, bbgn, bend, erate, MHAP_SLOP, st)
        if not ok:
            stats["nFailExtB"] += 1
        if st.alen == 1:
            stats["nFailExt"] += 1
            return
        o["ahg5"], o["ahg3"] = abgn, alen - aend
        o["bhg5"], o["bhg3"] = bbgn, blen - bend
        if partial:
            stats["nPartial"] += 1
            return
        if dovetail():
            stats["nDovetail"] += 1
            return
        ahg5, ahg3, bhg5, bhg3 = o["ahg5"], o["ahg3"], o["bhg5"], o["bhg3"]
        if ahg5 >= bhg5 and bhg5 > 0:
            ahg5 -= bhg5
            bhg5 = 0
            slop = int(bhg5 * erate + 100)
            abgn, aend, bbgn, bend = ahg5, alen - ahg3, bhg5, blen - bhg3
            ok, abgn, aend = _extend(B, bbgn, bend, A, abgn, aend, erate, slop, st)
            if ok:
                ahg5 = abgn
            else:
                ahg5, bhg5 = o["ahg5"], o["bhg5"]
            stats["nExt5b"] += 1
        if bhg5 >= ahg5 and ahg5 > 0:
            bhg5 -= ahg5
            ahg5 = 0
            slop = int(ahg5 * erate + 100)
            abgn, aend, bbgn, bend = ahg5, alen - ahg3, bhg5, blen - bhg3
            ok, bbgn, bend = _extend(A, abgn, aend, B, bbgn, bend, erate, slop, st)
            if ok:
                bhg5 = bbgn
            else:
                bhg5, ahg5 = o["bhg5"], o["ahg5"]
            stats["nExt5a"] += 1
        if bhg3 >= ahg3 and ahg3 > 0:
            bhg3 -= ahg3
            ahg3 = 0
            slop = int(ahg3 * erate + 100)
            abgn, aend, bbgn, bend = ahg5, alen - ahg3, bhg5, blen - bhg3
            ok, bbgn, bend = _extend(A, abgn, aend, B, bbgn, bend, erate, slop, st)
            if ok:
                bhg3 = blen - bend
            else:
                bhg3, ahg3 = o["bhg3"], o["ahg3"]
            stats["nExt3a"] += 1
        if ahg3 >= bhg3 and bhg3 > 0:
            ahg3 -= bhg3
            bhg3 = 0
            slop = int(bhg3 * erate + 100)
            abgn, aend, bbgn, bend = ahg5, alen - ahg3, bhg5, blen - bhg3
            ok, abgn, aend = _extend(B, bbgn, bend, A, abgn, aend, erate, slop, st)
            if ok:
                ahg3 = alen - aend
            else:
                ahg3, bhg3 = o["ahg3"], o["bhg3"]
            stats["nExt3b"] += 1
        o["ahg5"], o["ahg3"], o["bhg5"], o["bhg3"] = ahg5, ahg3, bhg5, bhg3
        # finalAlignment (:308-341)
        fa, fe, fb, fbe = ahg5, alen - ahg3, bhg5, blen - bhg3
        k = max_edit(fe - fa, fbe - fb, erate)
        d = global_align(A[fa:fe], B[fb:fbe], k)
        if d is not None:
            st.edit = d
            st.alen = align_len(fe - fa, fbe - fb, d)

    body()
    e_rate = st.edit / float(st.alen)
    if st.alen < min_len or e_rate > erate:
        stats["nFailed"] += 1
    else:
        stats["nPassed"] += 1
        o["evalue"] = encode_evalue(e_rate)
        o["forOBT"] = o["forDUP"] = int(bool(partial))
        o["forUTG"] = int((not partial) and dovetail())
    return o


def realign(records: np.ndarray, reads, erate: float, min_len: int, partial: bool = False,
            invert: bool = False):
    """(records, counters): `reads` maps a read ID to its bases (bytes)."""
    stats = {k: 0 for k in COUNTERS}
    out = np.zeros(records.shape[0], dtype=RECORD_DTYPE)
    for i, r in enumerate(records):
        o = realign_one(unpack(r), reads, erate, min_len, partial, invert, stats)
        out[i] = pack(o)
    return out, stats


def reads_dict(rs) -> dict:
    return {rs.first_iid + i: bytes(rs.read(i)) for i in range(rs.nreads)}


def parse_report(text: str) -> dict:
    """The counters out of alignStats::reportFinal's lines (overlapPair.C:138-153)."""
    import re
    pats = {
        "nSkipped": r"-- (\d+) skipped\.", "nFailed": r"-- (\d+) failed \d+ passed",
        "nPassed": r"-- \d+ failed (\d+) passed",
        "nFailExtA": r"-- (\d+) failed initial alignment, allowing A",
        "nFailExtB": r"-- (\d+) failed initial alignment, allowing B",
        "nFailExt": r"-- (\d+) failed initial alignment\n",
        "nPartial": r"-- (\d+) partial overlaps", "nDovetail": r"-- (\d+) dovetail overlaps",
        "nExt5a": r"-- (\d+)/\d+ A read", "nExt3a": r"-- \d+/(\d+) A read",
        "nExt5b": r"-- (\d+)/\d+ B read", "nExt3b": r"-- \d+/(\d+) B read"}
    return {k: int(re.search(p, text).group(1)) for k, p in pats.items()}


# ----------------------------------------------------------------------------- the fixtures

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("a", "b", "c", "d")


def parse_args(args: list[str]) -> dict:
    return {"erate": float(args[args.index("-erate") + 1]),
            "min_len": int(args[args.index("-len") + 1]),
            "partial": "-partial" in args, "invert": "-invert" in args}


_golden: dict = {}


def golden(name: str):
    """(reads, input records, the reference's output records, its counters, its options) of
    tests/golden/pair_<name>.npz (tools/make_pair_golden.py)."""
    if name not in _golden:
        from canu_amd.synth import ReadSet
        z = np.load(os.path.join(GOLDEN, f"pair_{name}.npz"))
        rs = ReadSet(bases=z["bases"], offsets=z["offsets"], lengths=z["lengths"], first_iid=1)
        inp = np.zeros(z["in_a"].shape[0], dtype=RECORD_DTYPE)
        out = np.zeros(z["out_a"].shape[0], dtype=RECORD_DTYPE)
        for f in RECORD_DTYPE.names:
            inp[f] = z["in_" + f]
            out[f] = z["out_" + f]
        for a in (inp, out, rs.bases, rs.offsets, rs.lengths):
            a.setflags(write=False)
        counters = dict(zip(COUNTERS, (int(v) for v in z["counters"])))
        args = z["args"].tobytes().decode().split()
        _golden[name] = (rs, inp, out, counters, args)
    return _golden[name]
