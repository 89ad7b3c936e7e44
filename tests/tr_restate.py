"""A Python restatement of canu's trimReads (src/overlapBasedTrimming/trimReads*.C,
clearRangeFile.H, trimStat.H, src/AS_UTL/intervalList.H), the checker of the GPU library on inputs
the reference was not run on.  tests/test_tr_cpu.py pins it to the reference's own .clear, .log,
.stats and stderr bytes (tests/golden/tr_*.npz, tools/make_tr_golden.py).

Two forms stand side by side.  The literal one is `IntervalList` (add, sort, merge, computeDepth
as the reference walks them) under `largest_covered`.  The closed one is what the kernel of
canu_amd/csrc/tr.hip computes: `closed_merge`, `closed_depth_runs`, `closed_intersect_best`
under `largest_covered_closed`.  The tests hold the two equal.

Overlap records are (a_iid, b_iid, w0, w1) in the ovOverlap layout; read i (1-based) has
lengths[i - 1] bases.  `branches`, where given, counts which paths ran.
"""
from __future__ import annotations

import struct

import numpy as np

HM = (1 << 21) - 1
EVALUE_SHIFT = 42
AS_MAX_EVALUE = 4095
U32 = 0xFFFFFFFF

NOT_IN_RANGE, NOV, DEL, NOC, MOD = 0, 1, 2, 3, 4
TAGS = {NOV: "NOV", DEL: "DEL", NOC: "NOC", MOD: "MOD"}
# trimReads.C:130-140, in the order the library returns them
COUNTERS = ("reads_in", "deleted_in", "no_trim_in", "reads_out", "no_ovl_out", "deleted_out",
            "no_change_out", "trim5", "trim3")
LOG_HEADER = "id\tinitL\tinitR\tfinalL\tfinalR\tmessage (DEL=deleted NOC=no change MOD=modified)\n"

# the branches the fixtures must reach (test_tr_cpu.py)
REQUIRED_BRANCHES = (
    "nov", "del_no_hq", "del_short", "noc", "mod", "skip_evalue",
    "merge_wrap", "merge_contained", "merge_thick", "merge_break", "merge_touch",
    "depth_merge_equal", "depth_merge_rewrites", "depth_low", "depth_gap_run",
    "isect_l_first", "isect_d_first", "isect_both_end", "isect_empty_pair",
    "longest_tie_first", "longest_later",
    "be_contained_twice", "be_break_066", "be_break_bound",
    "be_nibble", "be_nibble_refused", "be_skipped_scores", "be_outside_region")
# Not reachable, and so not required: "be_update_end_fails" (a score is its end minus the trim
# point, so a higher score at a point further in always ends further in) and "be_clamp" (every
# trim point lies within the largest covered region, and the nibble moves inwards).


class BadInput(ValueError):
    """Where the reference asserts or reads outside its arrays."""


def _bump(branches, key):
    if branches is not None:
        branches[key] = branches.get(key, 0) + 1


def encode_evalue(q: float) -> int:
    """AS_OVS_encodeEvalue, ovOverlap.H:44-45."""
    return int(10000.0 * q + 0.5) if q < AS_MAX_EVALUE / 10000.0 else AS_MAX_EVALUE


def decode_evalue(ev: int) -> float:
    return ev / 10000.0


def make_record(a: int, b: int, bgn: int, end: int, alen: int, evalue: int = 0,
                flags: int = 7) -> tuple:
    """An overlap of read a (alen bases) covering bgn..end, with b."""
    w0 = bgn | ((alen - end) << 21) | (evalue << EVALUE_SHIFT) | (flags << 55)
    return (a, b, w0, 0)


def spans(records, lengths):
    """-> a, b, a_bgn, a_end, evalue as int64 arrays (ovOverlap.H:235-236)."""
    a = records["a"].astype(np.int64)
    w0 = records["w0"]
    ln = np.asarray(lengths, dtype=np.int64)
    bad = (a < 1) | (a > ln.shape[0])
    if bad.any():
        raise BadInput(f"an overlap names read {int(a[bad][0])}; there are reads 1..{ln.shape[0]}")
    bgn = (w0 & np.uint64(HM)).astype(np.int64)
    end = ln[a - 1] - ((w0 >> np.uint64(21)) & np.uint64(HM)).astype(np.int64)
    ev = ((w0 >> np.uint64(EVALUE_SHIFT)) & np.uint64(0xFFF)).astype(np.int64)
    return a, records["b"].astype(np.int64), bgn, end, ev


# ------------------------------------------------------------------ intervalList, literally

class IntervalList:
    """intervalList<uint32>: entries [lo, hi, ct]; every value is 0."""

    def __init__(self):
        self.list: list[list[int]] = []
        self.is_sorted = True
        self.is_merged = True

    def add(self, position: int, length: int) -> None:                    # :232-255
        self.list.append([position, (position + length) & U32, 1])
        self.is_sorted = self.is_merged = False

    def sort(self) -> None:                                               # :259-275
        if self.is_sorted:
            return
        self.list.sort(key=lambda e: (e[0], e[1]))
        self.is_sorted = True

    def merge(self, min_overlap: int = 0, branches=None) -> None:         # :278-373
        if self.is_merged:
            return
        self.sort()
        L = self.list
        n = len(L)
        this, nxt = 0, 1
        while nxt < n:
            if L[this][0] == 0 and L[this][1] == 0:                       # :291-308
                L[this] = list(L[nxt])
                L[nxt][0] = L[nxt][1] = 0
                nxt += 1
                continue
            intersects = False
            if L[this][0] <= L[nxt][0] and L[nxt][1] <= L[this][1]:
                intersects = True
                _bump(branches, "merge_contained")
            if ((L[this][1] - min_overlap) & U32) >= L[nxt][0]:           # uint32 arithmetic
                intersects = True
                _bump(branches, "merge_wrap" if L[this][1] < min_overlap else "merge_thick")
            if intersects:
                if L[this][1] < L[nxt][1]:
                    L[this][1] = L[nxt][1]
                L[this][2] += L[nxt][2]
                L[nxt] = [0, 0, 0]
            else:
                _bump(branches, "merge_touch" if L[this][1] == L[nxt][0] else "merge_break")
                this += 1
                if this != nxt:
                    L[this] = list(L[nxt])
            nxt += 1
        if this + 1 < n:
            del L[this + 1:]
        self.is_merged = True

    @staticmethod
    def depth_of(src: "IntervalList", branches=None) -> "IntervalList":
        """intervalList(intervalList &IL): depth() and computeDepth(), :612-733."""
        ev = []
        for lo, hi, _ in src.list:
            ev.append((lo, True))
            ev.append((hi, False))
        out = IntervalList()
        out.is_sorted = out.is_merged = False
        if not ev:
            return out
        ev.sort(key=lambda e: (e[0], not e[1]))                           # pos, open first
        if not ev[0][1]:
            raise BadInput("the first depth event is a close")            # :665-668
        L = [[ev[0][0], ev[0][0], 1]]
        ll = 0                                                            # _listLen
        for i in range(1, len(ev)):
            pos, opn = ev[i]
            L[ll][1] = pos
            nct = L[ll][2] + (1 if opn else -1)
            if ev[i - 1][0] != pos and L[ll][0] != L[ll][1]:              # :695-703
                ll += 1
                if ll == len(L):
                    L.append([0, 0, 0])
                L[ll] = [pos, pos, L[ll - 1][2]]
            L[ll][1] = pos
            L[ll][2] = nct
            if ll > 1 and L[ll - 1][1] == L[ll][0] and L[ll - 1][2] == L[ll][2]:   # :712-718
                # the piece just opened falls back into the one before it; further closes at
                # this position then rewrite that piece's count
                L[ll - 1][1] = L[ll][1]
                ll -= 1
                _bump(branches, "depth_merge_equal")
                if i + 1 < len(ev) and ev[i + 1][0] == pos:
                    _bump(branches, "depth_merge_rewrites")
        out.list = [list(e) for e in L[:ll]]                              # the piece at ll is not counted
        return out


def depth_regions(IL: IntervalList, min_coverage: int, branches=None) -> IntervalList:
    """The ID loop of largestCovered, :93-141."""
    DE = IntervalList.depth_of(IL, branches)
    ID = IntervalList()
    ib = ie = 0
    for lo, hi, ct in DE.list:
        if ct < min_coverage:
            _bump(branches, "depth_low")
            if ie > ib:
                ID.add(ib, ie - ib)
                _bump(branches, "depth_gap_run")
            ib = ie = 0
        elif ib == 0 and ie == 0:
            ib, ie = lo, hi
        elif ie == lo:
            ie = hi
        else:
            if ie > ib:
                ID.add(ib, ie - ib)
            ib, ie = lo, hi
    if ie > ib:
        ID.add(ib, ie - ib)
    return ID


def intersect_walk(IL: IntervalList, ID: IntervalList, branches=None) -> IntervalList:
    """The two-pointer loop of largestCovered, :159-204."""
    FI = IntervalList()
    li = di = 0
    while li < len(IL.list) and di < len(ID.list):
        ll, lh = IL.list[li][0], IL.list[li][1]
        dl, dh = ID.list[di][0], ID.list[di][1]
        nl = nh = 0
        if ll <= dl and dl < lh:
            nl, nh = dl, (lh if lh < dh else dh)
        if dl <= ll and ll < dh:
            nl, nh = ll, (lh if lh < dh else dh)
        if nl < nh:
            FI.add(nl, nh - nl)
        else:
            _bump(branches, "isect_empty_pair")
        if lh <= dh:
            li += 1
        if dh <= lh:
            di += 1
        _bump(branches, "isect_both_end" if lh == dh else ("isect_l_first" if lh < dh else "isect_d_first"))
    return FI


def largest_covered(ivs, erate_value, min_overlap, min_coverage, branches=None):
    """largestCovered over the overlaps of one read; ivs: (bgn, end, evalue) in store order.
    -> (ok, fbgn, fend, n_skip, n_used); fbgn / fend are None when ok is False."""
    IL = IntervalList()
    n_skip = n_used = 0
    for bgn, end, ev in ivs:
        if not bgn < end:
            raise BadInput(f"an overlap of {bgn}..{end}")                 # :65
        if ev > erate_value:
            n_skip += 1
            _bump(branches, "skip_evalue")
            continue
        n_used += 1
        IL.add(bgn, end - bgn)
    if min_coverage > 0:
        ID = depth_regions(IL, min_coverage, branches)
    IL.merge(min_overlap, branches)
    if min_coverage > 0:
        IL = intersect_walk(IL, ID, branches)
    if not IL.list:
        return False, None, None, n_skip, n_used
    fbgn, fend = IL.list[0][0], IL.list[0][1]
    for k, (lo, hi, _) in enumerate(IL.list):
        if hi - lo > fend - fbgn:
            fbgn, fend = lo, hi
            _bump(branches, "longest_later")
        elif k and hi - lo == fend - fbgn:
            _bump(branches, "longest_tie_first")
    return True, fbgn, fend, n_skip, n_used


# ------------------------------------------------------------------ the closed forms

def closed_merge(pairs, min_overlap):
    """IL.merge(minOverlap) as one prefix-maximum scan: sorted by (lo, hi), a group breaks before
    interval i where neither the thick-overlap test (in uint32) nor containment holds against the
    maximum hi of everything before it."""
    iv = sorted(pairs)
    out = []
    pm = 0
    for i, (lo, hi) in enumerate(iv):
        if i == 0 or (not ((pm - min_overlap) & U32) >= lo and not hi <= pm):
            out.append([lo, hi])
        pm = max(pm, hi)
        out[-1][1] = pm
    return [tuple(e) for e in out]


def depth_needs_literal(pairs, min_coverage) -> bool:
    """computeDepth folds a just-opened piece back into its predecessor when, at one position,
    closes follow opens and the running count passes the predecessor's; more closes there then
    lower the predecessor's count below its true depth (IntervalList.depth_of).  That changes
    which pieces reach min_coverage only if the count ends below it, which needs an open and a
    close at one position and min_coverage >= 2.  The kernel tests exactly this and then walks
    the events literally."""
    if min_coverage < 2:
        return False
    los = {lo for lo, _ in pairs}
    return any(hi in los for _, hi in pairs)


def closed_depth_runs(pairs, min_coverage):
    """The maximal runs of positions covered by at least min_coverage intervals: a prefix sum of
    +1 / -1 over the sorted end points.  Equal to the reference's ID list unless
    depth_needs_literal()."""
    ev = sorted([(lo, 0) for lo, _ in pairs] + [(hi, 1) for _, hi in pairs])
    runs = []
    d = 0
    start = None
    for i, (pos, close) in enumerate(ev):
        d += -1 if close else 1
        if i + 1 < len(ev) and ev[i + 1][0] == pos:
            continue
        if d >= min_coverage and start is None:
            start = pos
        elif d < min_coverage and start is not None:
            runs.append((start, pos))
            start = None
    return runs


def closed_intersect_best(IL, ID):
    """The first strictly longest interval of the two-pointer walk without walking it: both lists
    ascend strictly in hi, so merged interval l meets exactly the depth runs d_first(l) ..
    d_last(l), d_last(l) the first run whose hi reaches l's, d_first(l) the run after
    d_last(l - 1) when their ends are equal and d_last(l - 1) itself otherwise."""
    dhi = [h for _, h in ID]
    best = None
    prev_last = None
    for l, (ll, lh) in enumerate(IL):
        if l == 0:
            first = 0
        else:
            first = prev_last + (1 if prev_last < len(ID) and dhi[prev_last] == IL[l - 1][1] else 0)
        last = int(np.searchsorted(np.array(dhi, dtype=np.int64), lh, side="left")) if dhi else 0
        prev_last = last
        for d in range(first, min(last, len(ID) - 1) + 1):
            dl, dh = ID[d]
            nl = nh = 0
            if ll <= dl and dl < lh:
                nl, nh = dl, min(lh, dh)
            if dl <= ll and ll < dh:
                nl, nh = ll, min(lh, dh)
            if nl < nh and (best is None or nh - nl > best[1] - best[0]):
                best = (nl, nh)
    return best


def largest_covered_closed(ivs, erate_value, min_overlap, min_coverage, branches=None):
    """largest_covered the way the kernel computes it."""
    used = [(b, e) for b, e, ev in ivs if ev <= erate_value]
    n_skip = len(ivs) - len(used)
    IL = closed_merge(used, min_overlap) if used else []
    if min_coverage > 0:
        if depth_needs_literal(used, min_coverage):
            lit = IntervalList()
            for b, e in used:
                lit.add(b, e - b)
            ID = [(lo, hi) for lo, hi, _ in depth_regions(lit, min_coverage).list]
        else:
            ID = closed_depth_runs(used, min_coverage)
        best = closed_intersect_best(IL, ID)
    else:
        best = None
        for lo, hi in IL:
            if best is None or hi - lo > best[1] - best[0]:
                best = (lo, hi)
    if best is None:
        return False, None, None, n_skip, len(used)
    return True, best[0], best[1], n_skip, len(used)


# ------------------------------------------------------------------ bestEdge

def best_edge(ovl, length, erate_value, min_overlap, min_coverage, branches=None,
              lc=largest_covered, ignore_b_iid=False):
    """bestEdge, trimReads-bestEdge.C:45-405; ovl: (bgn, end, evalue, b_iid) in store order,
    ibgn = 0 and iend = length.  -> (ok, fbgn, fend, n_skip, n_used, reset)."""
    ibgn, iend = 0, length
    ok, lbgn, lend, n_skip, n_used = lc([(b, e, v) for b, e, v, _ in ovl], erate_value, min_overlap,
                                        min_coverage, branches)
    if not ok:
        return False, ibgn, iend, n_skip, n_used, False
    trim5, trim3 = [], []
    n_contained = 0
    for tbgn, tend, ev, _ in ovl:                                         # :96-131
        if lend <= tbgn or tend <= lbgn:
            _bump(branches, "be_outside_region")
            continue
        if not tend <= iend:
            raise BadInput("an overlap past the end of its read")         # :107-108
        if ev > erate_value:
            continue
        if lbgn <= tbgn:
            trim5.append(tbgn)
        if tend <= lend:
            trim3.append(tend)
        if tbgn == ibgn and tend == iend:
            n_contained += 1
    if n_contained >= 2:
        trim5, trim3 = [], []
        _bump(branches, "be_contained_twice")
    trim5.append(lbgn)
    trim3.append(lend)
    trim5 = sorted(set(trim5))
    trim3 = sorted(set(trim3), reverse=True)

    best5pt = best5score = best5iid = best5end = 0
    for pt, triml in enumerate(trim5):                                    # :194-261
        score = sciid = scend = 0
        if best5score >= length - triml:
            _bump(branches, "be_break_bound")
            break
        for tbgn, tend, ev, b_iid in ovl:                                 # every overlap, :206
            if triml < tbgn or tend <= triml:
                continue
            if tend > lend:
                tend = lend
            tlen = tend - triml
            if score < tlen or (score == tlen and not ignore_b_iid and b_iid == best5iid):
                if ev > erate_value and score < tlen:
                    _bump(branches, "be_skipped_scores")
                score, sciid, scend = tlen, b_iid, tend
        if score < best5score * 0.66:
            _bump(branches, "be_break_066")
            break
        if best5score < score and best5end < scend:
            best5pt, best5score, best5iid, best5end = pt, score, sciid, scend
        elif best5score < score:
            _bump(branches, "be_update_end_fails")

    best3pt = best3score = best3iid = 0
    best3bgn = U32
    for pt, trimr in enumerate(trim3):                                    # :267-323
        score = sciid = scbgn = 0
        if best3score >= trimr:
            _bump(branches, "be_break_bound")
            break
        for tbgn, tend, ev, b_iid in ovl:
            if tend < trimr or trimr <= tbgn:
                continue
            if tbgn < lbgn:
                tbgn = lbgn
            tlen = trimr - tbgn
            if score < tlen or (score == tlen and not ignore_b_iid and b_iid == best3iid):
                if ev > erate_value and score < tlen:
                    _bump(branches, "be_skipped_scores")
                score, sciid, scbgn = tlen, b_iid, tbgn
        if score < best3score * 0.66:
            _bump(branches, "be_break_066")
            break
        if best3score < score and scbgn < best3bgn:
            best3pt, best3score, best3iid, best3bgn = pt, score, sciid, scbgn
        elif best3score < score:
            _bump(branches, "be_update_end_fails")

    fbgn, fend = trim5[best5pt], trim3[best3pt]                           # :377-399
    if fbgn + 4 < fend and 2 < fend:
        fbgn += 2
        fend -= 2
        _bump(branches, "be_nibble")
    else:
        _bump(branches, "be_nibble_refused")
    if fbgn < lbgn:
        fbgn = lbgn
        _bump(branches, "be_clamp")
    if lend < fend:
        fend = lend
        _bump(branches, "be_clamp")
    reset = False
    if fend < fbgn:
        fbgn, fend, reset = lbgn, lend, True
    return True, fbgn, fend, n_skip, n_used, reset


# ------------------------------------------------------------------ the per-read loop

class Params:
    def __init__(self, erate=0.015, min_read_length=64, min_evidence_overlap=40,
                 min_evidence_coverage=1):
        self.erate = erate
        self.min_read_length = min_read_length
        self.min_evidence_overlap = min_evidence_overlap
        self.min_evidence_coverage = min_evidence_coverage


def trim_reads(lengths, records, rules, P: Params, id_range=None, branches=None, closed=False,
               ignore_b_iid=False) -> dict:
    """trimReads.C:257-437.  rules: 0 / 1 / 2 for every read, or one number.  id_range: -t, inclusive.
    closed=True computes largestCovered the kernel's way."""
    ln = np.asarray(lengths, dtype=np.int64)
    n = ln.shape[0]
    rl = np.broadcast_to(np.asarray(rules, dtype=np.int64), (n,))
    a, b, bgn, end, ev = spans(records, ln)
    if a.shape[0] and (np.diff(a) < 0).any():
        raise BadInput("the overlaps are not sorted by a_iid")
    id_min, id_max = id_range if id_range is not None else (1, U32)
    id_min = max(id_min, 1)
    id_max = min(id_max, n)
    ev_max = encode_evalue(P.erate)
    off = np.searchsorted(a, np.arange(1, n + 2))
    R = {"bgn": np.zeros(n, np.uint32), "end": ln.astype(np.uint32), "status": np.zeros(n, np.uint8),
         "n_skipped": np.zeros(n, np.uint32), "n_used": np.zeros(n, np.uint32),
         "no_hq": np.zeros(n, np.uint8), "reset": np.zeros(n, np.uint8),
         "id_min": id_min, "id_max": id_max, "lengths": ln.astype(np.uint32)}
    C = {k: [0, 0] for k in COUNTERS}

    def count(k, bases):
        C[k][0] += 1
        C[k][1] += int(bases)

    lc = largest_covered_closed if closed else largest_covered
    for rid in range(id_min, id_max + 1):
        i = rid - 1
        L = int(ln[i])
        count("reads_in", L)
        s, e = int(off[i]), int(off[i + 1])
        ibgn, iend = 0, L
        fbgn, fend = ibgn, iend
        good = False
        if e > s:
            ov = [(int(bgn[k]), int(end[k]), int(ev[k]), int(b[k])) for k in range(s, e)]
            if rl[i] == 1:
                good, fb, fe, nsk, nus = lc([o[:3] for o in ov], ev_max, P.min_evidence_overlap,
                                            P.min_evidence_coverage, branches)
                if good:
                    fbgn, fend = fb, fe
            elif rl[i] == 2:
                good, fbgn, fend, nsk, nus, rs = best_edge(ov, L, ev_max, P.min_evidence_overlap,
                                                           P.min_evidence_coverage, branches, lc,
                                                           ignore_b_iid)
                R["reset"][i] = rs
            else:
                raise BadInput(f"read {rid} with overlaps has trimming rule {int(rl[i])}")   # :352-356
            R["n_skipped"][i], R["n_used"][i], R["no_hq"][i] = nsk, nus, not good
        elif rl[i] not in (1, 2):
            raise BadInput(f"read {rid} has trimming rule {int(rl[i])}")
        R["bgn"][i], R["end"][i] = fbgn, fend
        if e == s:                                                        # :375-387
            count("no_ovl_out", L)
            R["status"][i] = NOV
            _bump(branches, "nov")
        elif not good or fend - fbgn < P.min_read_length:                 # :389-401
            count("deleted_out", L)
            R["status"][i] = DEL
            _bump(branches, "del_short" if good else "del_no_hq")
        elif ibgn == fbgn and iend == fend:                               # :405-415
            count("no_change_out", L)
            R["status"][i] = NOC
            _bump(branches, "noc")
        else:                                                             # :419-436
            count("reads_out", fend - fbgn)
            R["status"][i] = MOD
            _bump(branches, "mod")
            if fbgn - ibgn > 0:
                count("trim5", fbgn - ibgn)
            if iend - fend > 0:
                count("trim3", iend - fend)
    R["counters"] = {k: tuple(v) for k, v in C.items()}
    return R


# ------------------------------------------------------------------ the output texts

def clear_bytes(R: dict, existing: bytes | None = None) -> bytes:
    """The -Co file (clearRangeFile.H:87-99): uint32 numReads, bgn[numReads + 1], end[numReads + 1].
    An existing file is loaded, reset to 0..length (entry 0 keeps what the file held), then
    written over."""
    ln = R["lengths"]
    n = ln.shape[0]
    bgn = np.zeros(n + 1, dtype="<u4")
    end = np.zeros(n + 1, dtype="<u4")
    if existing is not None:
        obgn, oend = parse_clear(existing, n)
        bgn[0], end[0] = obgn[0], oend[0]
    end[1:] = ln
    st = R["status"]
    gone = (st == NOV) | (st == DEL)
    mod = st == MOD
    bgn[1:][gone] = U32
    end[1:][gone] = U32
    bgn[1:][mod] = R["bgn"][mod]
    end[1:][mod] = R["end"][mod]
    return struct.pack("<I", n) + bgn.tobytes() + end.tobytes()


def parse_clear(raw: bytes, num_reads: int | None = None):
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


def log_text(R: dict) -> str:
    out = [LOG_HEADER]
    ln = R["lengths"]
    for i in range(R["id_min"] - 1, R["id_max"]):
        st = int(R["status"][i])
        if st == NOV:
            msg = ""
        elif R["no_hq"][i]:
            msg = "\tno high quality overlaps"
        else:
            msg = f"\tskipped {int(R['n_skipped'][i])} overlaps; used {int(R['n_used'][i])} overlaps"
        out.append(f"{i + 1}\t0\t{int(ln[i])}\t{int(R['bgn'][i])}\t{int(R['end'][i])}\t{TAGS[st]}{msg}\n")
    return "".join(out)


def stats_text(R: dict, P: Params) -> str:
    """trimReads.C:469-504."""
    c = R["counters"]

    def row(k, what):
        return "%6u reads %12u bases (%s)\n" % (c[k][0], c[k][1], what)

    return ("PARAMETERS:\n----------\n"
            "%7u    (reads trimmed below this many bases are deleted)\n" % P.min_read_length +
            "%7.4f    (use overlaps at or below this fraction error)\n" % decode_evalue(encode_evalue(P.erate)) +
            "%7u    (break region if overlap is less than this long, for 'largest covered' algorithm)\n"
            % P.min_evidence_overlap +
            "%7u    (break region if overlap coverage is less than this many read%s, for 'largest covered' algorithm)\n"
            % (P.min_evidence_coverage, "" if P.min_evidence_coverage == 1 else "s") +
            "\nINPUT READS:\n-----------\n" +
            row("reads_in", "reads processed") +
            row("deleted_in", "reads not processed, previously deleted") +
            row("no_trim_in", "reads not processed, in a library where trimming isn't allowed") +
            "\nOUTPUT READS:\n------------\n" +
            row("reads_out", "trimmed reads output") +
            row("no_change_out", "reads with no change, kept as is") +
            row("no_ovl_out", "reads with no overlaps, deleted") +
            row("deleted_out", "reads with short trimmed length, deleted") +
            "\nTRIMMING DETAILS:\n----------------\n" +
            row("trim5", "bases trimmed from the 5' end of a read") +
            row("trim3", "bases trimmed from the 3' end of a read"))


def stderr_text(R: dict) -> str:
    """The "Processing" line (trimReads.C:262-265) and bestEdge's "iid" lines (:396)."""
    out = [f"Processing from ID {R['id_min']} to {R['id_max']} out of {R['lengths'].shape[0]} reads.\n"]
    out += [f"iid = {i + 1}\n" for i in np.flatnonzero(R["reset"])]
    return "".join(out)


# ------------------------------------------------------------------ the hand-made cases

# What tools/make_tr_golden.py puts on the reads of fixtures b (rule 1) and c (rule 2), and what
# tests/test_gpu_tr.py moves to random positions.
BAD_EV = 500                                           # 5 %: beyond -e 0.015

# name -> intervals (bgn, end[, evalue]) on a read of 1000 bases
CASES_B = [
    ("wrap", [(0, 30), (500, 900)]),
    ("touching", [(0, 400), (400, 800)]),
    ("identical", [(100, 600)] * 3),
    ("contained_thin", [(100, 600), (570, 590)]),
    ("thin_overlap_deep", [(0, 500), (10, 510), (480, 900), (490, 950)]),
    ("depth_hole", [(0, 400)] * 3 + [(300, 700)] + [(600, 1000)] * 3),
    ("two_winners", [(0, 300), (500, 800)]),
    ("all_skipped", [(0, 900, BAD_EV), (50, 950, BAD_EV)]),
    ("some_skipped", [(0, 900, BAD_EV), (50, 700), (60, 720)]),
    ("minlength_m1", [(100, 163)]),
    ("minlength", [(100, 164)]),
    ("depth_rewrite", [(0, 300), (100, 300), (300, 400)]),
    ("later_longer", [(0, 100), (300, 900)]),
    ("full", [(0, 1000)]),
    ("full_twice", [(0, 1000), (0, 1000)]),
    ("walk_back", [(0, 100), (62, 200), (0, 95), (97, 200), (0, 95), (97, 200)]),
]

# rule 2
CASES_C = [
    ("issue_example", [(0, 700), (50, 1000), (200, 960)]),
    ("contained_twice", [(0, 1000), (0, 1000), (100, 800)]),
    ("break_066", [(0, 600), (300, 1000), (500, 1000), (800, 1000)]),
    ("nibble_refused", [(100, 104)]),
    ("skipped_scores", [(0, 1000, BAD_EV), (100, 600), (300, 900)]),
    ("outside_region", [(0, 50), (200, 1000), (250, 950)]),
    ("one", [(20, 980)]),
    ("stairs", [(0, 400), (100, 500), (200, 600), (300, 700), (400, 800), (500, 900), (600, 1000)]),
    ("crossing", [(0, 520), (480, 1000), (500, 510)]),
    ("no_hq", [(0, 900, BAD_EV)]),
]
