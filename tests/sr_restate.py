"""A Python restatement of canu's splitReads (src/overlapBasedTrimming/splitReads*.C,
adjustNormal.C, adjustFlipped.C, clearRangeFile.H, trimStat.H, src/AS_UTL/intervalList.H), the
checker of the GPU library on inputs the reference was not run on.  tests/test_sr_cpu.py pins it to
the reference's own .clear, .log, .stats and stderr bytes (tests/golden/sr_*.npz,
tools/make_sr_golden.py).

Overlap records are (a_iid, b_iid, w0, w1) in the ovOverlap layout, sorted by (a_iid, b_iid); read
i (1-based) has lengths[i - 1] bases and library switches lib_flags[i - 1].  `branches`, where
given, counts which paths ran.

Two forms of the interval work stand side by side: the literal `IntervalList` walk (merge with
counts, invert) and the closed forms the kernel of canu_amd/csrc/sr.hip computes
(`closed_merge_counts`, `closed_largest_good`).  The tests hold them equal.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from tr_restate import IntervalList as _TrIntervalList

HM = (1 << 21) - 1
AS_MAX_READLEN = HM
U32 = 0xFFFFFFFF
FLIPPED_BIT = 54

LIB_ELIGIBLE, LIB_SUBREADS = 1, 2

# the status of a read
NOT_IN_RANGE, DELETED_IN, NO_TRIM, NO_OVERLAPS, NO_COVERAGE, NO_CHANGE, TRIMMED, DELETED_OUT = range(8)
# the fate of a record
F_NOT_IN_RANGE, F_DROPPED, F_KEPT, F_MANY, F_SAME_ORIENT = range(5)

SUBREAD_LOOP_MAX_SIZE = 500                            # splitReads.H
SUBREAD_LOOP_EXT_SIZE = 2000

# the trimStat of splitReads.C:64-114 the .stats file prints, in the order the library returns them
COUNTERS = ("reads_in", "deleted_in", "no_trim_in", "no_overlaps", "no_coverage", "proc_chimera",
            "proc_spur", "proc_subread", "reads_bad_spur5", "reads_bad_spur3", "reads_bad_chimera",
            "reads_bad_subread", "bases_bad_spur5", "bases_bad_spur3", "bases_bad_chimera",
            "bases_bad_subread", "trimmed5", "trimmed3", "no_change", "deleted_out")

# the branches the fixtures must reach (test_sr_cpu.py)
REQUIRED_BRANCHES = (
    "deleted_in", "no_trim", "no_overlaps", "no_coverage", "no_change", "trimmed", "deleted_out",
    "not_subread_lib", "drop_deleted_b", "miss_a_clear", "miss_b_clear",
    "snap_bgn_full", "snap_bgn_limited", "snap_end_full", "snap_end_limited", "adjust_half",
    "group_one", "group_many", "pair_same_orient", "pair_disjoint", "palindrome",
    "pair_a_strong", "pair_b_weak", "bad_small", "bad_ext_only", "bad_too_far", "bad_zero_length",
    "bad_swapped", "tie_takes_jj", "merge_fuse", "merge_touch", "merge_break",
    "span_reject", "span_nine_kept", "span_margin_lo", "span_margin_hi", "weak_reject",
    "confirm_count", "confirm_allhits", "confirm_palindrome",
    "largest_tie_first", "largest_later", "two_regions", "whole_bad", "flipped", "range_clamped")


class BadInput(ValueError):
    """Where the reference asserts or computes on a wrapped value."""


class Params:
    def __init__(self, erate=0.015, min_read_length=64):
        self.erate = erate
        self.min_read_length = min_read_length


def _bump(branches, key, by=1):
    if branches is not None:
        branches[key] = branches.get(key, 0) + by


def make_record(a, b, a_bgn, a_end, alen, b_bgn, b_end, blen, flipped=False, evalue=0, flags=4):
    """An overlap of a_bgn..a_end on read a (alen bases) with b_bgn..b_end on read b, the B
    coordinates on the reverse complement when flipped (what adjustFlipped computes back)."""
    w0 = a_bgn | ((alen - a_end) << 21) | (evalue << 42) | (int(bool(flipped)) << FLIPPED_BIT) | (flags << 55)
    w1 = b_bgn | ((blen - b_end) << 21)
    return (a, b, w0, w1)


def c_round(x: float) -> int:
    """C's round() on a non-negative double: half away from zero.  (floor(x + 0.5) is wrong for
    the double just below one half, whose sum with 0.5 rounds up to 1.)"""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f


# ------------------------------------------------------------------ intervalList<int32>

class IntervalList(_TrIntervalList):
    """tr_restate's list (add, sort, merge with counts) and invert, intervalList.H:409-463.  All
    values here are non-negative and below 2^31, where the int32 and the uint32 list agree."""

    def invert(self, invlo: int, invhi: int) -> None:
        self.merge()
        L = self.list
        inv = []
        if not L:
            inv.append([invlo, invhi, 1])
        else:
            if invlo < L[0][0]:
                inv.append([invlo, L[0][0], 1])
            for i in range(1, len(L)):
                if L[i - 1][1] < L[i][0]:
                    inv.append([L[i - 1][1], L[i][0], 1])
            if L[-1][1] < invhi:
                inv.append([L[-1][1], invhi, 1])
        self.list = inv


def closed_merge_counts(pairs):
    """IL.merge(0) with counts the way the kernel does it: sorted by (lo, hi); the leading (0, 0)
    intervals fall away unless there is nothing else (intervalList.H:291-308 copies the next
    interval over an empty one, count and all); a group breaks before an interval whose lo lies
    beyond every hi before it.  -> [(lo, hi, count)]"""
    iv = sorted(pairs)
    nz = 0
    while nz < len(iv) and iv[nz] == (0, 0):
        nz += 1
    if iv and nz == len(iv):
        return [(0, 0, 1)]
    out = []
    for lo, hi in iv[nz:]:
        if out and out[-1][1] >= lo:
            out[-1][1] = max(out[-1][1], hi)
            out[-1][2] += 1
        else:
            out.append([lo, hi, 1])
    return [tuple(e) for e in out]


def closed_largest_good(regions, clr_bgn, clr_end):
    """trimBadInterval's inversion and choice without the list: regions are merged intervals in
    order (hi < next lo); a leading (0, 0) before another region is what merge() drops.
    -> (bgn, end), 0, 0 where no good piece has a positive size."""
    r = list(regions)
    if len(r) > 1 and r[0][:2] == (0, 0):
        r = r[1:]
    pieces = []
    if not r:
        pieces.append((clr_bgn, clr_end))
    else:
        if clr_bgn < r[0][0]:
            pieces.append((clr_bgn, r[0][0]))
        for k in range(1, len(r)):
            pieces.append((r[k - 1][1], r[k][0]))
        if r[-1][1] < clr_end:
            pieces.append((r[-1][1], clr_end))
    best = (0, 0)
    for lo, hi in pieces:
        if hi - lo > best[1] - best[0]:
            best = (lo, hi)
    return best


# ------------------------------------------------------------------ one overlap

def decode(rec, lengths):
    """-> a, b, flipped, aovlbgn, aovlend, bovlbgn, bovlend (B on the strand the overlap uses:
    adjustFlipped's bLen - b_bgn() is bhg5 again), ovOverlap.H:235-239."""
    a, b, w0, w1 = int(rec[0]), int(rec[1]), int(rec[2]), int(rec[3])
    la, lb = int(lengths[a - 1]), int(lengths[b - 1])
    return (a, b, (w0 >> FLIPPED_BIT) & 1, w0 & HM, la - ((w0 >> 21) & HM), w1 & HM, lb - ((w1 >> 21) & HM))


def adjust(abgn, aend, bbgn, bend, acb, ace, bcb, bce, branches=None):
    """adjustNormal.C:57-123 / adjustFlipped.C:60-126 after the coordinates are gathered, then the
    two 15-base snaps of splitReads-workUnit.C:95-130.  -> None where the overlap misses a clear
    range, else the four adjusted coordinates."""
    if ace <= abgn or aend <= acb:
        _bump(branches, "miss_a_clear")
        return None
    if bce <= bbgn or bend <= bcb:
        _bump(branches, "miss_b_clear")
        return None
    alen, blen = aend - abgn, bend - bbgn
    afb = (0 if acb < abgn else acb - abgn) / alen
    bfb = (0 if bcb < bbgn else bcb - bbgn) / blen
    afe = (0 if ace > aend else aend - ace) / alen
    bfe = (0 if bce > bend else bend - bce) / blen
    mb, me = max(afb, bfb), max(afe, bfe)
    if not (mb < 1.0 and me < 1.0):
        raise BadInput("an overlap trimmed away whole")                   # adjustNormal.C:90-91
    for x in (mb * alen, mb * blen, me * alen, me * blen):
        if x - math.floor(x) == 0.5:
            _bump(branches, "adjust_half")
    abgn += c_round(mb * alen)
    bbgn += c_round(mb * blen)
    aend -= c_round(me * alen)
    bend -= c_round(me * blen)
    if not (acb <= abgn and bcb <= bbgn and aend <= ace and bend <= bce) or aend < 0 or bend < 0:
        raise BadInput("an adjusted overlap outside its clear range")     # :118-121
    if bbgn - bcb < 15:
        limit, adj = abgn - acb, bbgn - bcb
        if adj > limit:
            adj = limit
            _bump(branches, "snap_bgn_limited")
        elif adj > 0:
            _bump(branches, "snap_bgn_full")
        abgn -= adj
        bbgn -= adj
    if bce - bend < 15:
        limit, adj = ace - aend, bce - bend
        if adj > limit:
            adj = limit
            _bump(branches, "snap_end_limited")
        elif adj > 0:
            _bump(branches, "snap_end_full")
        aend += adj
        bend += adj
    return abgn, aend, bbgn, bend


def _isect(b1, e1, b2, e2):
    lo, hi = max(b1, b2), min(e1, e2)
    return hi - lo if hi > lo else 0


def detect_subreads(adj, b_sub, fate, branches=None, closed=False):
    """splitReads-subReads.C:67-308.  adj: [(record index, b_iid, flipped, abgn, aend, bbgn,
    bend)] in input order; b_sub(b_iid): the B read's library checks subreads.  Sets fate of the
    records the ERROR lines name.  -> the confirmed regions [(lo, hi)]."""
    groups: dict = {}
    for k, o in enumerate(adj):
        groups.setdefault(o[1], []).append(k)
    palindrome = False
    bad, bad_all = [], []
    for k, o in enumerate(adj):
        g = groups[o[1]]
        if len(g) == 1:
            _bump(branches, "group_one")
            continue
        if len(g) > 2:
            fate[o[0]] = F_MANY
            _bump(branches, "group_many")
            continue
        if k == g[1]:
            continue
        p = adj[g[1]]
        if o[2] == p[2]:
            fate[o[0]] = F_SAME_ORIENT
            _bump(branches, "pair_same_orient")
            continue
        a_ov = _isect(o[3], o[4], p[3], p[4])
        b_ov = _isect(o[5], o[6], p[5], p[6])
        if a_ov == 0 and b_ov == 0:
            _bump(branches, "pair_disjoint")
            continue
        if a_ov > 1000 and b_ov > 1000 and b_sub(o[1]):
            palindrome = True
            _bump(branches, "palindrome")
        if a_ov > 250 or b_ov < 250:
            _bump(branches, "pair_a_strong" if a_ov > 250 else "pair_b_weak")
            continue
        if o[3] < p[3]:
            lo, hi = o[4], p[3]
        else:
            lo, hi = p[4], o[3]
            if o[3] == p[3]:
                _bump(branches, "tie_takes_jj")
        if lo > hi:
            lo, hi = hi, lo
            _bump(branches, "bad_swapped")
        if hi == lo:
            _bump(branches, "bad_zero_length")
        if hi - lo <= SUBREAD_LOOP_MAX_SIZE:
            bad.append((lo, hi))
            _bump(branches, "bad_small")
        elif hi - lo <= SUBREAD_LOOP_EXT_SIZE:
            _bump(branches, "bad_ext_only")
        else:
            _bump(branches, "bad_too_far")
        if hi - lo <= SUBREAD_LOOP_EXT_SIZE:
            bad_all.append((lo, hi))

    def merged(pairs):
        if closed:
            return closed_merge_counts(pairs)
        L = IntervalList()
        for lo, hi in pairs:
            L.add(lo, hi - lo)
        L.merge(0)
        return [tuple(e) for e in L.list]

    if branches is not None:
        s = sorted(bad)
        pm = None
        for lo, hi in s:
            if pm is not None:
                _bump(branches, "merge_touch" if pm == lo else ("merge_fuse" if pm > lo else "merge_break"))
            pm = hi if pm is None else (max(pm, hi) if pm >= lo else hi)
    BAD, ALL = merged(bad), merged(bad_all)
    regions = []
    for lo, hi, ct in BAD:
        all_hits = sum(c for alo, ahi, c in ALL if alo <= lo and hi <= ahi)
        n_span = sum(1 for o in adj if o[3] + 100 < lo and hi + 100 < o[4])
        if branches is not None:
            if any(o[3] + 100 == lo and hi + 100 < o[4] for o in adj):
                _bump(branches, "span_margin_lo")
            if any(o[3] + 100 < lo and hi + 100 == o[4] for o in adj):
                _bump(branches, "span_margin_hi")
        if n_span > 9:
            _bump(branches, "span_reject")
            continue
        if ct + all_hits // 4 + int(palindrome) < 3:
            _bump(branches, "weak_reject")
            continue
        if n_span == 9:
            _bump(branches, "span_nine_kept")
        if ct >= 3:
            _bump(branches, "confirm_count")
        elif ct + all_hits // 4 >= 3:
            _bump(branches, "confirm_allhits")
        else:
            _bump(branches, "confirm_palindrome")
        regions.append((lo, hi))
    return regions


def trim_bad_interval(regions, clr_bgn, clr_end, branches=None, closed=False):
    """splitReads-trimBad.C:40-78 on a non-empty list.  -> (bgn, end)"""
    if closed:
        return closed_largest_good(regions, clr_bgn, clr_end)
    good = IntervalList()
    for lo, hi in regions:
        good.add(lo, hi - lo)
    good.invert(clr_bgn, clr_end)
    bgn = end = 0
    for k, (lo, hi, _) in enumerate(good.list):
        if ((end - bgn) & U32) < ((hi - lo) & U32):                       # uint32 against int32
            if k:
                _bump(branches, "largest_later")
            bgn, end = lo, hi
        elif k and hi - lo == end - bgn:
            _bump(branches, "largest_tie_first")
    if not good.list or end == bgn:
        _bump(branches, "whole_bad")
    return bgn, end


# ------------------------------------------------------------------ the per-read loop

def normalize_clear(lengths, clear):
    ln = np.asarray(lengths, dtype=np.int64)
    if clear is None:
        return np.zeros(ln.shape[0], np.int64), ln.copy()
    cb, ce = (np.asarray(c, dtype=np.int64) for c in clear)
    if cb.shape != ln.shape or ce.shape != ln.shape:
        raise BadInput("clear ranges for another number of reads")
    return cb, ce


def validate(ln, records, cb, ce):
    """What sr_split_reads answers with SR_ERR_BAD_INPUT."""
    n = ln.shape[0]
    if (ln > AS_MAX_READLEN).any():
        raise BadInput("a read beyond AS_MAX_READLEN")
    live = ~((cb == U32) & (ce == U32))
    if ((cb > ce) | (ce > ln))[live].any():
        raise BadInput("a clear range outside its read")
    a, b = records["a"].astype(np.int64), records["b"].astype(np.int64)
    if ((a < 1) | (a > n) | (b < 1) | (b > n)).any():
        raise BadInput(f"an overlap names a read outside 1..{n}")
    if a.shape[0] > 1:
        key = (a << 32) | b
        if (np.diff(key) < 0).any():
            raise BadInput("the overlaps are not sorted by (a_iid, b_iid)")
    w0, w1 = records["w0"], records["w1"]
    m, s = np.uint64(HM), np.uint64(21)
    if (((w0 & m) + ((w0 >> s) & m)).astype(np.int64) >= ln[a - 1]).any():
        raise BadInput("an overlap with a_bgn >= a_end")
    if (((w1 & m) + ((w1 >> s) & m)).astype(np.int64) >= ln[b - 1]).any():
        raise BadInput("an overlap with b_bgn >= b_end")


def split_reads(lengths, records, lib_flags, clear, params, id_range=None, branches=None,
                closed=False) -> dict:
    """splitReads.C:221-373.  lib_flags: LIB_ELIGIBLE | LIB_SUBREADS per read, or one number.
    clear: None (0 .. length) or (bgn, end) per read, UINT32_MAX twice for a deleted read.
    id_range: -t, inclusive."""
    ln = np.asarray(lengths, dtype=np.int64)
    n = ln.shape[0]
    lf = np.broadcast_to(np.asarray(lib_flags, dtype=np.int64), (n,))
    cb, ce = normalize_clear(ln, clear)
    validate(ln, records, cb, ce)
    id_min, id_max = id_range if id_range is not None else (1, U32)
    if id_min < 1 or id_max > n:
        _bump(branches, "range_clamped")
    id_min, id_max = max(id_min, 1), min(id_max, n)
    a_ids = records["a"].astype(np.int64)
    off = np.searchsorted(a_ids, np.arange(1, n + 2))
    deleted = (cb == U32) & (ce == U32)
    R = {"bgn": cb.astype(np.uint32), "end": ce.astype(np.uint32), "status": np.zeros(n, np.uint8),
         "n_adjusted": np.zeros(n, np.uint32), "n_bad_regions": np.zeros(n, np.uint32),
         "fate": np.zeros(records.shape[0], np.uint8), "regions": [], "region_off": np.zeros(n + 1, np.uint64),
         "id_min": id_min, "id_max": id_max, "lengths": ln.astype(np.uint32),
         "clear_in": (cb.astype(np.uint32), ce.astype(np.uint32))}
    C = {k: [0, 0] for k in COUNTERS}

    def count(k, bases):
        C[k][0] += 1
        C[k][1] += int(bases)

    fate = R["fate"]
    for rid in range(id_min, id_max + 1):
        i = rid - 1
        L = int(ln[i])
        if deleted[i]:
            count("deleted_in", L)
            R["status"][i] = DELETED_IN
            _bump(branches, "deleted_in")
            continue
        if not lf[i] & LIB_ELIGIBLE:
            count("no_trim_in", L)
            R["status"][i] = NO_TRIM
            _bump(branches, "no_trim")
            continue
        count("reads_in", L)
        s, e = int(off[i]), int(off[i + 1])
        if s == e:
            count("no_overlaps", L)
            R["status"][i] = NO_OVERLAPS
            _bump(branches, "no_overlaps")
            continue
        acb, ace = int(cb[i]), int(ce[i])
        adj = []
        for k in range(s, e):
            _, b, flipped, abgn, aend, bbgn, bend = decode(records[k], ln)
            fate[k] = F_DROPPED
            if deleted[b - 1]:
                _bump(branches, "drop_deleted_b")
                continue
            lb = int(ln[b - 1])
            if flipped:
                _bump(branches, "flipped")
                bcb, bce = lb - int(ce[b - 1]), lb - int(cb[b - 1])
            else:
                bcb, bce = int(cb[b - 1]), int(ce[b - 1])
            got = adjust(abgn, aend, bbgn, bend, acb, ace, bcb, bce, branches)
            if got is None:
                continue
            fate[k] = F_KEPT
            adj.append((k, b, flipped) + got)
        R["n_adjusted"][i] = len(adj)
        if not adj:
            count("no_coverage", L)
            R["status"][i] = NO_COVERAGE
            _bump(branches, "no_coverage")
            continue
        regions = []
        if lf[i] & LIB_SUBREADS:
            count("proc_subread", L)
            regions = detect_subreads(adj, lambda b: bool(lf[b - 1] & LIB_SUBREADS), fate, branches, closed)
        else:
            _bump(branches, "not_subread_lib")
        R["n_bad_regions"][i] = len(regions)
        R["regions"] += [(rid, lo, hi) for lo, hi in regions]
        if not regions:
            count("no_change", L)
            R["status"][i] = NO_CHANGE
            _bump(branches, "no_change")
            continue
        if len(regions) > 1:
            _bump(branches, "two_regions")
        for lo, hi in regions:
            count("bases_bad_subread", hi - lo)
        count("reads_bad_subread", len(regions))
        bgn, end = trim_bad_interval(regions, acb, ace, branches, closed)
        if not (bgn >= acb and ace >= end):
            raise BadInput(f"read {rid}: a clear range that grew")        # splitReads.C:365-366
        R["bgn"][i], R["end"][i] = bgn, end
        if end - bgn < (params.min_read_length & U32):
            count("deleted_out", L)
            R["status"][i] = DELETED_OUT
            _bump(branches, "deleted_out")
        else:
            R["status"][i] = TRIMMED
            _bump(branches, "trimmed")
        if bgn > acb:
            count("trimmed5", bgn - acb)
        if ace > end:
            count("trimmed3", ace - end)
    R["region_off"][1:] = np.cumsum(R["n_bad_regions"])
    R["counters"] = {k: tuple(v) for k, v in C.items()}
    return R


# ------------------------------------------------------------------ the output texts

def parse_clear(raw: bytes, num_reads=None):
    """-> (bgn, end), each numReads + 1 long."""
    if len(raw) < 4:
        raise ValueError(f"a clear range file of {len(raw)} bytes has no read count")
    (n,) = struct.unpack("<I", raw[:4])
    if num_reads is not None and n != num_reads:
        raise ValueError(f"a clear range file for {n} reads, the store has {num_reads}")
    if len(raw) != 4 + 8 * (n + 1):
        raise ValueError(f"a clear range file of {len(raw)} bytes does not hold its {n} reads")
    v = np.frombuffer(raw, dtype="<u4", offset=4)
    return v[:n + 1].copy(), v[n + 1:].copy()


def clear_ranges(R: dict):
    """The output clear range of every read: the input's, the trimmed one, or deleted."""
    bgn, end = R["clear_in"][0].copy(), R["clear_in"][1].copy()
    t = R["status"] == TRIMMED
    bgn[t], end[t] = R["bgn"][t], R["end"][t]
    d = R["status"] == DELETED_OUT
    bgn[d] = end[d] = U32
    return bgn, end


def clear_bytes(R: dict, entry0=(0, 0)) -> bytes:
    """The -Co file (clearRangeFile.H:87-99).  Whatever it held is reset and then overwritten
    from -Ci (splitReads.C:188-195), entry 0 included: entry0 is the -Ci file's, 0, 0 without."""
    bgn, end = clear_ranges(R)
    n = bgn.shape[0]
    return struct.pack("<I", n) + struct.pack("<I", entry0[0]) + bgn.astype("<u4").tobytes() + \
        struct.pack("<I", entry0[1]) + end.astype("<u4").tobytes()


def log_text(R: dict) -> str:
    """subreadFile is never opened: logMsg stays empty (splitReads-trimBad.C:82)."""
    return ""


def stats_text(R: dict, P: Params) -> str:
    """splitReads.C:409-445."""
    c = R["counters"]

    def row(k, what, unit="bases"):
        return "%6u reads %12u %s (%s)\n" % (c[k][0], c[k][1], unit, what)

    return ("PARAMETERS:\n----------\n"
            "%7u    (reads trimmed below this many bases are deleted)\n" % (P.min_read_length & U32) +
            "%7.4f    (use overlaps at or below this fraction error)\n" % P.erate +
            "INPUT READS:\n-----------\n" +
            row("reads_in", "reads processed") +
            row("deleted_in", "reads not processed, previously deleted") +
            row("no_trim_in", "reads not processed, in a library where trimming isn't allowed") +
            "\nPROCESSED:\n--------\n" +
            row("no_overlaps", "no overlaps") +
            row("no_coverage", "no coverage after adjusting for trimming done already") +
            row("proc_chimera", "processed for chimera") +
            row("proc_spur", "processed for spur") +
            row("proc_subread", "processed for subreads") +
            "\nREADS WITH SIGNALS:\n------------------\n" +
            row("reads_bad_spur5", "number of 5' spur signal", "signals") +
            row("reads_bad_spur3", "number of 3' spur signal", "signals") +
            row("reads_bad_chimera", "number of chimera signal", "signals") +
            row("reads_bad_subread", "number of subread signal", "signals") +
            "\nSIGNALS:\n-------\n" +
            row("bases_bad_spur5", "size of 5' spur signal") +
            row("bases_bad_spur3", "size of 3' spur signal") +
            row("bases_bad_chimera", "size of chimera signal") +
            row("bases_bad_subread", "size of subread signal") +
            "\nTRIMMING:\n--------\n" +
            row("trimmed5", "trimmed from the 5' end of the read") +
            row("trimmed3", "trimmed from the 3' end of the read"))


def stderr_text(R: dict, P: Params, records) -> str:
    """The "Processing" line (splitReads.C:226-230) and detectSubReads' ERROR lines."""
    out = ["Processing from ID %u to %u out of %u reads, using errorRate = %.2f\n"
           % (R["id_min"], R["id_max"], R["lengths"].shape[0], P.erate)]
    for k in np.flatnonzero(R["fate"] >= F_MANY):
        a, b = int(records["a"][k]), int(records["b"][k])
        out.append(f"ERROR: more overlaps than expected for pair {a} {b}.\n" if R["fate"][k] == F_MANY
                   else f"ERROR: same orient duplicate overlaps for pair {a} {b}\n")
    return "".join(out)
