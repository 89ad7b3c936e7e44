"""A Python restatement of canu's findErrors (src/overlapErrorAdjustment/), the checker of the
GPU library on inputs the reference was not run on.  tests/test_fe_cpu.py pins it to the
reference's own .red bytes (tests/golden/fe_*.npz, tools/make_fe_golden.py).

Bases are codes 0..3 = acgt; every byte outside ACGTacgt is 'a' (findErrors-Read_Frags.C:46-54,
findErrors.C:74-82).  Edit_Match_Limit comes from oracle.match_limit (Binomial_Bound.C:116, the
restatement the overlapInCore checker already uses; findErrors hands it the double error rate).
"""
from __future__ import annotations

import math
import os

import numpy as np

MAX_DEGREE = 32767                      # findErrors.H:87
MAX_VOTE = 255                          # findErrors.H:90
MIN_HAPLO_OCCURS = 3                    # findErrors.H:102
BRANCH_PT_MATCH_VALUE = 0.272           # findErrors.H:57
AS_MAX_READLEN = (1 << 21) - 1

# Vote_Value_t, correctionOutput.H:24-37
IDENT, DELETE, A_SUBST, C_SUBST, G_SUBST, T_SUBST, A_INSERT, C_INSERT, G_INSERT, T_INSERT = \
    range(10)
# columns of a read's tally, Vote_Tally_t (findErrors.H:111-125)
CONFIRMED, DELETES, SUBST0, NO_INSERT, INSERT0 = 0, 1, 2, 6, 7
HM = (1 << 21) - 1

RED_DTYPE = np.dtype([("word", "<u4"), ("readID", "<u4")])

_FILTER = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _FILTER[ord(_c)] = _FILTER[ord(_c.lower())] = _i


def filter_read(b) -> np.ndarray:
    """findErrors-Read_Frags.C:46-54 and :111-112."""
    return _FILTER[np.frombuffer(bytes(b), dtype=np.uint8)]


def defaults() -> dict:
    """feParameters(), findErrors.H:304-337."""
    return {"erate": 0.06, "degree_threshold": 2, "kmer_len": 9, "vote_qualify_len": 9,
            "end_exclude_len": 3, "use_haplo_ct": True}


def parse_args(args: list[str]) -> dict:
    """main()'s options, findErrors.C:381-425 (the ones that change the result)."""
    o = defaults()
    i = 0
    while i < len(args):
        a = args[i]
        if a == "-p":
            o["use_haplo_ct"] = False
        else:
            v = args[i + 1]
            i += 1
            if a == "-e":
                o["erate"] = float(v)
            elif a == "-d":
                o["degree_threshold"] = int(v)
            elif a == "-k":
                o["kmer_len"] = int(v)
            elif a == "-V":
                o["vote_qualify_len"] = int(v)
            elif a == "-x":
                o["end_exclude_len"] = int(v)
        i += 1
    return o


def error_bound(i: int, erate: float) -> int:
    """findErrors.C:476-477."""
    return int(math.ceil(i * erate))


_ml: dict = {}


def match_limit(erate: float, n: int) -> np.ndarray:
    """Edit_Match_Limit[0..n), findErrors.C:472-474."""
    import oracle
    key = float(erate)
    if key not in _ml or _ml[key].shape[0] < n:
        max_errors = 1 + int(erate * AS_MAX_READLEN)
        _, lim = oracle.match_limit(key, min(max(n, 64), max_errors))
        _ml[key] = lim
    return _ml[key]


# ------------------------------------------------------------------------- the aligner

class _Rows:
    """Edit_Array_Lazy as the aligner leaves it: row e holds its values on the pruned band
    [lo, hi] and the -2 the next row wrote around it (Prefix_Edit_Distance.C:216-219)."""

    def __init__(self):
        self.lo, self.hi, self.base, self.val = [], [], [], []

    def push(self, base, val, lo, hi):
        self.base.append(base)
        self.val.append(val)
        self.lo.append(lo)
        self.hi.append(hi)

    def get(self, e, d):
        if self.lo[e] <= d <= self.hi[e]:
            return int(self.val[e][d - self.base[e]])
        return -2


def compute_delta(R: _Rows, e: int, d: int, row: int) -> list[int]:
    """Compute_Delta, findErrors-Prefix_Edit_Distance.C:30-76."""
    last = row
    stack = []
    for k in range(e, 0, -1):
        frm = d
        mx = 1 + R.get(k - 1, d)
        j = R.get(k - 1, d - 1)
        if j > mx:
            frm, mx = d - 1, j
        j = 1 + R.get(k - 1, d + 1)
        if j > mx:
            frm, mx = d + 1, j
        if frm == d - 1:
            stack.append(mx - last - 1)
            d -= 1
            last = R.get(k - 1, frm)
        elif frm == d + 1:
            stack.append(last - (mx - 1))
            d += 1
            last = R.get(k - 1, frm)
    stack.append(last + 1)
    sign = lambda v: (v > 0) - (v < 0)
    return [abs(stack[i]) * sign(stack[i - 1]) for i in range(len(stack) - 1, 0, -1)]


_AR = np.arange(32)


def _slide(Ap, Tp, row, ds):
    act = np.arange(row.shape[0])
    while act.size:
        idx = row[act][:, None] + _AR
        eq = Ap[idx] == Tp[idx + ds[act][:, None]]
        full = eq.all(axis=1)
        adv = np.where(full, 32, np.argmin(eq, axis=1))
        row[act] += adv
        act = act[full]


def prefix_edit_dist(A, T, limit: int, erate: float, ML, stats=None):
    """Prefix_Edit_Dist, findErrors-Prefix_Edit_Distance.C:166-309.
    -> (errors, a_end, t_end, match_to_end, delta)."""
    m, n = A.shape[0], T.shape[0]
    shorter = min(m, n)
    ne = np.nonzero(A[:shorter] != T[:shorter])[0]
    row0 = int(ne[0]) if ne.size else shorter
    if row0 == shorter:                                                   # :195-200
        return 0, row0, row0, True, []
    Ap = np.concatenate([A, np.full(40, 254, np.uint8)])
    Tp = np.concatenate([T, np.full(40, 255, np.uint8)])
    R = _Rows()
    R.push(0, np.array([row0], dtype=np.int64), 0, 0)
    left = right = 0
    best_d = best_e = longest = 0
    max_score = 0.0
    ms_len = ms_d = ms_e = 0
    used = 1                                  # entries of the edit array written so far
    for e in range(1, limit + 1):
        left = max(left - 1, -e)
        right = min(right + 1, e)
        ds = np.arange(left, right + 1)
        P = np.full(right - left + 3, -2, dtype=np.int64)     # row e-1 on [left-1, right+1]
        lo, hi, b = R.lo[e - 1], R.hi[e - 1], R.base[e - 1]
        P[lo - (left - 1):hi - (left - 1) + 1] = R.val[e - 1][lo - b:hi - b + 1]
        row = np.maximum(np.maximum(1 + P[1:-1], P[:-2]), P[2:] + 1)
        _slide(Ap, Tp, row, ds)
        if stats is not None:
            stats["rows"] += 1
            used += right - left + 1
            stats["max_width"] = max(stats.get("max_width", 0), right - left + 1)
            stats["log_used"] = max(stats.get("log_used", 0), used)
        end = np.nonzero((row == m) | (row + ds == n))[0]
        if end.size:                                                      # :233-250
            k = int(end[0])
            d, r = int(ds[k]), int(row[k])
            if r == m and 1 + R.get(e - 1, d + 1) == r and d < right:
                d += 1
            R.push(left, row, left, right)
            return e, r, r + d, True, compute_delta(R, e, d, r)
        lim = int(ML[e])
        g = lambda d: int(row[d - ds[0]])
        while left <= right and left < 0 and g(left) < lim:                # :253-271
            left += 1
        if left >= 0:
            while left <= right and g(left) + left < lim:
                left += 1
        if left > right:
            R.push(int(ds[0]), row, left, right)
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
        if int(seg[k]) > longest:                                         # :275-280
            best_d, best_e, longest = left + k, e, int(seg[k])
        score = int(longest * BRANCH_PT_MATCH_VALUE - e)                  # int32: truncated
        if score > max_score and \
                best_e <= error_bound(min(longest, longest + best_d), erate):
            max_score = float(score)
            ms_len, ms_d, ms_e = longest, best_d, best_e
    return ms_e, ms_len, ms_len + ms_d, False, compute_delta(R, ms_e, ms_d, ms_len)


# --------------------------------------------------------------------------- the votes

def _vote(T, col, pos):
    if T[pos, col] < MAX_VOTE:                                            # Cast_Vote, :42-69
        T[pos, col] += 1


def analyze_alignment(T, A, a_part, a_len, a_offset, b_part, delta, P, stats=None):
    """Analyze_Alignment, findErrors-Analyze_Alignment.C:100-293.  T: the A read's tallies.
    `stats`, if a dict, counts in "outside" the matching-base votes that fall outside the read
    (the reference writes them to whatever lies there), collects in "runs" the lengths of the
    match runs that vote when kmer_len < 2 * end_exclude_len (where the first and third vote
    loops can overlap) and counts in "fs_skipped" the changes :282 keeps from voting."""
    gv = [(-1, -1, A_SUBST)]                                              # frag_sub, align_sub, vote
    i = j = p = 0

    def run(L):
        nonlocal i, j, p
        if L <= 0:
            return
        for k in np.nonzero(a_part[i:i + L] != b_part[j:j + L])[0]:
            gv.append((i + int(k), p + int(k), A_SUBST + int(b_part[j + int(k)])))
        i += L
        j += L
        p += L

    for dl in delta:
        run(abs(dl) - 1)
        if dl < 0:
            gv.append((i - 1, p, A_INSERT + int(b_part[j])))
            j += 1
            p += 1
        if dl > 0:
            gv.append((i, p, DELETE))
            i += 1
            p += 1
    run(a_len - i)
    ct = len(gv)
    gv.append((i, p, None))
    K, V, X = P["kmer_len"], P["vote_qualify_len"], P["end_exclude_len"]
    for c in range(1, ct + 1):
        prev_match = gv[c][1] - gv[c - 1][1] - 1
        p_lo = 0 if c == 1 else X
        p_hi = prev_match if c == ct else prev_match - X
        f0 = gv[c - 1][0]
        if prev_match >= K:                                               # :246-270
            # the first and third loops exactly as written: with kmer_len < 2 end_exclude_len
            # they overlap, and can step outside the run; outside the read there is no tally
            if stats is not None and K < 2 * X:
                stats.setdefault("runs", set()).add((prev_match, c == 1, c == ct, a_offset > 0))
            for q in list(range(0, p_lo)) + list(range(p_hi, prev_match)):
                k = a_offset + f0 + q + 1
                if 0 <= k < T.shape[0]:
                    _vote(T, SUBST0 + int(A[k]), k)
                elif stats is not None:
                    stats["outside"] = stats.get("outside", 0) + 1
            if p_hi > p_lo:
                k0 = a_offset + f0 + p_lo + 1
                k1 = a_offset + f0 + p_hi + 1
                T[k0:k1, CONFIRMED] = np.minimum(T[k0:k1, CONFIRMED] + 1, MAX_VOTE)
                T[k0:k1 - 1, NO_INSERT] = np.minimum(T[k0:k1 - 1, NO_INSERT] + 1, MAX_VOTE)
        if c < ct and (prev_match > 0 or gv[c - 1][2] <= T_SUBST or gv[c][2] <= T_SUBST):
            next_match = gv[c + 1][1] - gv[c][1] - 1
            fs = a_offset + gv[c][0]
            if fs < 0 or fs >= a_len:                                     # :282, a_len: a quirk
                if stats is not None:
                    stats["fs_skipped"] = stats.get("fs_skipped", 0) + 1
                continue
            if prev_match + next_match >= V:
                col = DELETES if gv[c][2] == DELETE else \
                    SUBST0 + gv[c][2] - A_SUBST if gv[c][2] <= T_SUBST else \
                    INSERT0 + gv[c][2] - A_INSERT
                _vote(T, col, fs)


# ----------------------------------------------------------------------------- the job

def unpack_olap(rec):
    """a_iid, b_iid, a_hang, b_hang, flipped of an ovOverlap record (ovOverlap.H:227-228)."""
    w0, w1 = int(rec["w0"]), int(rec["w1"])
    ahg5, ahg3, bhg5, bhg3 = w0 & HM, (w0 >> 21) & HM, w1 & HM, (w1 >> 21) & HM
    return int(rec["a"]), int(rec["b"]), ahg5 - bhg5, bhg3 - ahg3, (w0 >> 54) & 1


def make_record(a, b, a_hang, b_hang, flipped):
    ahg5, bhg5 = max(a_hang, 0), max(-a_hang, 0)
    bhg3, ahg3 = max(b_hang, 0), max(-b_hang, 0)
    return (a, b, ahg5 | (ahg3 << 21) | (int(bool(flipped)) << 54) | (1 << 57),
            bhg5 | (bhg3 << 21))


def find_errors(records, reads: dict, bgn: int, end: int, P: dict, stats=None):
    """Read_Olaps .. Output_Corrections -> (.red records, passed, failed).  reads: id -> bytes.
    `stats`, if a dict, receives rows and bases aligned, and the tallies (read -> one row of
    Vote_Tally_t per base) and degrees (read -> [left, right]) the decision is made from."""
    erate = P["erate"]
    seqs = {}

    def seq(i):
        if i not in seqs:
            seqs[i] = filter_read(reads[i])
        return seqs[i]

    tallies = {i: np.zeros((len(reads[i]), 11), dtype=np.int32) for i in range(bgn, end + 1)}
    deg = {i: [0, 0] for i in range(bgn, end + 1)}
    passed = failed = 0
    if stats is not None:
        stats.setdefault("rows", 0)
        stats.setdefault("bases", 0)
    maxlen = max([len(r) for r in reads.values()] + [1])
    ML = match_limit(erate, error_bound(maxlen, erate) + 2)
    for rec in records:
        a, b, a_hang, b_hang, flipped = unpack_olap(rec)
        assert bgn <= a <= end
        A = seq(a)
        B = seq(b)
        if flipped:
            B = (3 - B)[::-1]
        a_offset = max(a_hang, 0)                                         # Process_Olap :93-101
        a_part = A[a_offset:]
        b_part = B[max(-a_hang, 0):]
        if a_hang <= 0 and deg[a][0] < MAX_DEGREE:
            deg[a][0] += 1
        if b_hang >= 0 and deg[a][1] < MAX_DEGREE:
            deg[a][1] += 1
        olap_len = min(a_part.shape[0], b_part.shape[0])
        errors, a_end, b_end, to_end, delta = prefix_edit_dist(
            a_part, b_part, error_bound(olap_len, erate), erate, ML, stats)
        if stats is not None:
            stats["bases"] += olap_len
        if not to_end and a_end + a_offset >= A.shape[0] - 1:             # :149-152
            olap_len = min(a_end, b_end)
            to_end = True
            if stats is not None:
                stats["rescued"] = stats.get("rescued", 0) + 1
        if errors <= error_bound(olap_len, erate) and to_end:
            passed += 1
            analyze_alignment(tallies[a], A, a_part, a_end, a_offset, b_part, delta, P, stats)
        else:
            failed += 1
    if stats is not None:
        stats["tallies"] = tallies
        stats["degrees"] = deg
    return output_corrections(tallies, deg, seqs, reads, bgn, end, P), passed, failed


def output_corrections(tallies, deg, seqs, reads, bgn, end, P):
    """Output_Corrections, findErrors-Output.C:49-234."""
    out = []
    hap = P["use_haplo_ct"]
    for rid in range(bgn, end + 1):
        keep = (deg[rid][0] < P["degree_threshold"]) | ((deg[rid][1] < P["degree_threshold"]) << 1)
        out.append((keep, rid))
        T = tallies[rid]
        if T.shape[0] == 0:
            continue
        S = seqs[rid] if rid in seqs else filter_read(reads[rid])
        for j in np.nonzero(T[:, 1:].any(axis=1))[0]:
            t = [int(v) for v in T[j]]
            j = int(j)
            if t[CONFIRMED] < 2:
                vote, mx, is_change = DELETE, t[DELETES], True
                for c in range(4):
                    if t[SUBST0 + c] > mx:
                        vote, mx, is_change = A_SUBST + c, t[SUBST0 + c], int(S[j]) != c
                five = [t[DELETES]] + t[SUBST0:SUBST0 + 4]
                haplo = sum(v >= MIN_HAPLO_OCCURS for v in five)
                total = sum(five)
                if total <= 1 or 2 * mx <= total or not is_change or (haplo >= 2 and hap) or \
                        (t[CONFIRMED] > 0 and (t[CONFIRMED] != 1 or mx <= 6)):
                    continue                          # the reference's `continue`: no insert test
                out.append((keep | (vote << 2) | (j << 6), rid))
            if t[NO_INSERT] < 2:
                ins, imx = A_INSERT, t[INSERT0]
                for c in range(1, 4):
                    if imx < t[INSERT0 + c]:
                        ins, imx = A_INSERT + c, t[INSERT0 + c]
                four = t[INSERT0:INSERT0 + 4]
                ihap = sum(v >= MIN_HAPLO_OCCURS for v in four)
                itot = sum(four)
                if itot <= 1 or 2 * imx >= itot or (ihap >= 2 and hap) or \
                        (t[NO_INSERT] > 0 and (t[NO_INSERT] != 1 or imx <= 6)):
                    continue
                out.append((keep | (ins << 2) | (j << 6), rid))
    return np.array(out, dtype=RED_DTYPE) if out else np.zeros(0, dtype=RED_DTYPE)


# ----------------------------------------------------------------------------- the fixtures

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("a", "b", "c", "d", "e", "f", "g", "h", "i")
_golden: dict = {}


def reads_dict(rs) -> dict:
    return {rs.first_iid + i: bytes(rs.read(i)) for i in range(rs.nreads)}


def golden(name: str):
    """(reads, store records of the range, the reference's .red records, passed, failed, bgn,
    end, its options) of tests/golden/fe_<name>.npz (tools/make_fe_golden.py)."""
    if name not in _golden:
        from canu_amd.overlap_in_core import RECORD_DTYPE
        from canu_amd.synth import ReadSet
        z = np.load(os.path.join(GOLDEN, f"fe_{name}.npz"))
        rs = ReadSet(bases=z["bases"], offsets=z["offsets"], lengths=z["lengths"], first_iid=1)
        inp = np.zeros(z["in_a"].shape[0], dtype=RECORD_DTYPE)
        for f in RECORD_DTYPE.names:
            inp[f] = z["in_" + f]
        red = np.frombuffer(z["red"].tobytes(), dtype=RED_DTYPE)
        for a in (inp, rs.bases, rs.offsets, rs.lengths):
            a.setflags(write=False)
        args = z["args"].tobytes().decode().split()
        c = [int(v) for v in z["counters"]]
        _golden[name] = (rs, inp, red, c[0], c[1], c[2], c[3], args)
    return _golden[name]
