"""A vote builder for findErrors: B reads and overlap records that put a wanted Vote_Tally_t at a
chosen base of an A read, the constructed cases of the two Output_Corrections ladders, and the
ladders once more with a counter on every branch.

How a B read votes (findErrors-Analyze_Alignment.C:239-292, tests/fe_restate.py):

  * a piece that matches A over a run of at least kmer_len bases adds `confirmed` to the run
    without its end_exclude_len bases next to a change, and `no_insert` to the same bases but
    the last; the excluded bases get a vote for A's own letter instead.  The alignment's two
    ends are no changes: a piece that ends in base j confirms j and leaves its no_insert alone.
  * a piece with a substitution or deletion at j, or an inserted letter behind j, adds that
    vote when the matches before and behind it reach vote_qualify_len -- and when
    a_offset + j < the aligned length of A (:282 compares with the wrong length), so a piece
    that starts at base lo of A votes only on changes at j < hi - lo.  A piece made for base j
    therefore spans [j - W, 2j - W] or so, and sites that share an A read lie about twice as
    deep each as the one before, never only kmer_len + 2 * end_exclude_len + vote_qualify_len
    apart; most cases take a short A read of their own.
  * the aligner moves an indel to the right end of a run of one letter: a deletion of A[j]
    lands on j when A[j + 1] differs, an inserted letter behind j when it is not A[j + 1].

With end_exclude_len 0 nothing votes for A's own letter, so `!is_change` cannot happen there:
a vote for a letter is a mismatch of the alignment, and the only other source is the excluded
bases.  With it above 0 an inserting piece votes A's own letter at j as well, so the insert
ladder of a base is reached only through a substitution or delete record that outvotes them.
"""
from __future__ import annotations

import collections

import numpy as np

import fe_restate as FR

_ACGT = b"ACGT"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

# the option lines of the fixtures e..i (tools/make_fe_golden.py)
LINES = {
    "e": ["-e", "0.06"],
    "f": ["-e", "0.06", "-p"],
    "g": ["-e", "0.06", "-k", "8", "-V", "6", "-x", "0"],
    "h": ["-e", "0.06", "-k", "4", "-x", "5", "-V", "2"],
    "i": ["-e", "0.06", "-k", "8", "-V", "6", "-x", "0", "-p"],
}


def _rc(b: bytes) -> bytes:
    return b.translate(_COMP)[::-1]


def T(c=0, d=0, s=(0, 0, 0, 0), ni=0, i=(0, 0, 0, 0)) -> list:
    """A tally in Vote_Tally_t order (findErrors.H:111-125)."""
    return [c, d, *s, ni, *i]


class Lab:
    def __init__(self, seed: int, args):
        self.args = list(args)
        self.P = FR.parse_args(self.args)
        self.rng = np.random.default_rng(seed)
        self.a_reads: list[bytes] = []
        self.pieces: list = []                    # A index, B read, a_hang, b_hang, flipped
        self.want: list = []                      # A index, base, tally
        K, V, X = self.P["kmer_len"], self.P["vote_qualify_len"], self.P["end_exclude_len"]
        self.W = K + X + 1                        # a run that votes, and 2 W >= V in every line
        self.apart = K + 2 * X + V
        assert 2 * self.W >= V

    def rand(self, n: int) -> bytes:
        return np.frombuffer(_ACGT, dtype=np.uint8)[self.rng.integers(0, 4, n)].tobytes()

    def add_a(self, n: int, sites: dict | None = None) -> int:
        """A random A read; sites: base -> (its letter, the next base's letter) as codes."""
        a = bytearray(self.rand(n))
        for j, (own, nxt) in (sites or {}).items():
            a[j] = _ACGT[own]
            if j + 1 < n:
                a[j + 1] = _ACGT[nxt]
        self.a_reads.append(bytes(a))
        return len(self.a_reads) - 1

    def piece(self, a: int, lo: int, hi: int, edits=(), lead: bytes = b"", trail: bytes = b"",
              copies: int = 1) -> None:
        """B = lead + A[lo:hi] with edits + trail.  edits: (base, "S" | "D" | "I", letter code);
        "I" puts the letter behind the base.  B reads alternate forward and flipped."""
        A = self.a_reads[a]
        n = len(A)
        assert 0 <= lo < hi <= n and (not lead or lo == 0) and (not trail or hi == n)
        ed = collections.defaultdict(list)
        for pos, op, c in edits:
            assert lo <= pos < hi and op in "SDI"
            ed[pos].append((op, c))
        out = bytearray(lead)
        for pos in range(lo, hi):
            ops = dict(ed.get(pos, []))
            if "S" in ops:
                assert _ACGT[ops["S"]] != A[pos]
                out.append(_ACGT[ops["S"]])
            elif "D" not in ops:
                out.append(A[pos])
            if "I" in ops:
                out.append(_ACGT[ops["I"]])
        out += trail
        for _ in range(copies):
            self.pieces.append((a, bytes(out), lo - len(lead), len(trail) - (n - hi),
                                len(self.pieces) & 1))

    def false_pair(self, a: int) -> None:
        """An overlap the reads do not have: it fails."""
        n = len(self.a_reads[a])
        self.pieces.append((a, self.rand(n), 0, 0, len(self.pieces) & 1))

    def expect(self, a: int, j: int, tally) -> None:
        self.want.append((a, j, [int(v) for v in tally]))

    def site(self, a: int, j: int, tally, lo: int | None = None) -> None:
        """Pieces that put exactly `tally` at base j of A read a; ValueError where no set of
        pieces can.  lo: where the pieces start in A (default j - W; 0 for a deep base)."""
        c, d, s, ni, ins = tally[0], tally[1], list(tally[2:6]), tally[6], list(tally[7:11])
        A = self.a_reads[a]
        n, X, W = len(A), self.P["end_exclude_len"], self.W
        own = _ACGT.index(A[j])
        n_ins = sum(ins)
        near = s[own] - (n_ins if X else 0)       # an inserting piece excludes j: A's own letter
        ends = c - ni - (0 if X else n_ins)       # with -x 0 it confirms j
        if near < 0 or ends < 0 or (near and not X):
            raise ValueError(f"no pieces give {tally} with end_exclude_len {X}")
        if (n_ins or d or ni) and j + 1 >= n:
            raise ValueError("the last base takes substitutions and `confirmed` only")
        if n_ins and ins[_ACGT.index(A[j + 1])]:
            raise ValueError("an inserted letter equal to the next base lands one base on")
        if d and A[j + 1] == A[j]:
            raise ValueError("a deletion in a run of one letter lands on the run's last base")
        lo = max(0, j - W) if lo is None else lo

        def change(at, edit, copies):
            hi = min(n, at + max(W, lo) + 1)
            if copies and at >= hi - lo:
                raise ValueError(f":282 keeps a piece from base {lo} from voting at {at}")
            if copies:
                self.piece(a, lo, hi, [edit], copies=copies)

        if ni:
            self.piece(a, lo, min(n, j + W + 1), copies=ni)
        if ends:
            self.piece(a, lo, j + 1, copies=ends)
        for k in range(4):
            if k != own:
                change(j, (j, "S", k), s[k])
            change(j, (j, "I", k), ins[k])
        change(j, (j, "D", 0), d)
        for k in range(near):                     # a substitution end_exclude_len away
            at = j + X if j + X + self.P["kmer_len"] < n else j - X
            assert lo <= at
            change(at, (at, "S", (_ACGT.index(A[at]) + 1 + k % 3) % 4), 1)
        self.expect(a, j, tally)

    def single(self, tally, own: int = 0, nxt: int = 3) -> int:
        """A short A read of its own with the site at base W + 1; its pieces start at base 1, so
        they add to no degree."""
        j = self.W + 1
        a = self.add_a(2 * self.W + 4, {j: (own, nxt)})
        self.site(a, j, tally, lo=1)
        return a

    def job(self, order=None):
        """-> (reads, overlap records, bgn, end): the A reads are the range, the B reads follow."""
        n_a = len(self.a_reads)
        reads = list(self.a_reads)
        recs = []
        for k, (a, b, ah, bh, fl) in enumerate(self.pieces):
            reads.append(_rc(b) if fl else b)
            recs.append(FR.make_record(a + 1, n_a + 1 + k, ah, bh, fl))
        if order is not None:
            recs = [recs[i] for i in order]
        return reads, recs, 1, n_a

    def check(self, stats: dict) -> None:
        """The precondition of every comparison: each site carries the tally it was built for, by
        the restatement's own tallies, and no vote fell outside a read (where the reference
        writes into the next read's tallies)."""
        assert stats.get("outside", 0) == 0
        for a, j, want in self.want:
            got = [int(v) for v in stats["tallies"][a + 1][j]]
            assert got == want, (a + 1, j, got, want)


def restate(lab: Lab, order=None):
    """-> (reads, records, bgn, end, .red records, passed, failed, stats) by the restatement,
    with the lab's preconditions checked."""
    from canu_amd.overlap_in_core import RECORD_DTYPE
    reads, recs, bgn, end = lab.job(order)
    st: dict = {}
    red, p, f = FR.find_errors(np.array(recs, dtype=RECORD_DTYPE),
                               {i + 1: r for i, r in enumerate(reads)}, bgn, end, lab.P, st)
    lab.check(st)
    return reads, recs, bgn, end, red, p, f, st


# ------------------------------------------------------------------------------ the cases

def substitution(lab: Lab) -> None:
    X = lab.P["end_exclude_len"]
    lab.single(T(s=(0, 1, 0, 0)))                             # total 1
    lab.single(T(s=(0, 2, 0, 0)))                             # total 2: a record
    lab.single(T(s=(0, 2, 2, 0)))                             # 2 max == total, two letters tied
    lab.single(T(d=1, s=(0, 1, 0, 0)))                        # the same with delete: it keeps it
    lab.single(T(d=2, s=(0, 0, 0, 2)))
    lab.single(T(s=(0, 3, 2, 0)))                             # 2 max == total + 1: a record
    lab.single(T(d=3, s=(0, 0, 2, 0)))                        # a delete record
    lab.single(T(s=(0, 0, 4, 2)))                             # the second value at 2: a record
    lab.single(T(s=(0, 0, 4, 3)))                             # at MIN_HAPLO_OCCURS: only with -p
    lab.single(T(d=3, s=(0, 4, 0, 0)))
    if X:
        lab.single(T(s=(3, 1, 0, 0)))                         # A's own letter wins: !is_change
        lab.single(T(s=(0, 2, 3, 1)), own=2, nxt=0)
    for c in (0, 1, 2):
        for m in (6, 7):
            lab.single(T(c=c, s=(0, 0, 0, m)), own=1, nxt=0)
    # three sites of one A read, each twice as deep as the one before and `apart` more
    j1 = lab.W + 1
    j2 = 2 * j1 + lab.apart
    j3 = 2 * j2 + lab.apart
    a = lab.add_a(2 * j3 + 2, {j1: (0, 3), j2: (1, 3), j3: (2, 3)})
    lab.site(a, j1, T(s=(0, 2, 0, 0)))
    lab.site(a, j2, T(c=1, d=7))
    lab.site(a, j3, T(s=(0, 3, 0, 2)))


def insert(lab: Lab) -> None:
    X, hap = lab.P["end_exclude_len"], lab.P["use_haplo_ct"]

    def site(ni, i, own=0, nxt=3):
        """The insert ladder is reached: with -x 0 through `confirmed` (each inserting piece
        confirms the base), else through a substitution record that outvotes the inserting
        pieces' votes for A's own letter."""
        n = sum(i)
        if X == 0:
            lab.single(T(c=max(2, n + ni), ni=ni, i=i), own, nxt)
        else:
            s = [0, 0, 0, 0]
            s[own], s[(own + 1) % 4] = n, n + 1
            lab.single(T(c=ni, s=s, ni=ni, i=i), own, nxt)

    site(0, (1, 0, 0, 0))                                     # ins_total 1
    site(0, (1, 1, 0, 0))                                     # ins_total 2, 2 ins_max == ins_total
    if X == 0 or not hap:
        site(0, (2, 1, 1, 0))                                 # 2 ins_max == ins_total
        site(0, (2, 2, 1, 0))                                 # one below, tied: a keeps it
        site(0, (1, 2, 2, 0))                                 # tied: c keeps it
        site(0, (0, 1, 1, 1), own=2, nxt=0)
        site(0, (3, 3, 1, 0))                                 # ins_haplo_ct 2
        site(0, (3, 2, 2, 0))                                 # ins_haplo_ct 1
    if not hap:                                               # 7 + 4 + 4: three letters at 3
        for ni in (0, 1, 2):
            for m in (6, 7):
                site(ni, (m, 4, 4, 0))


def interaction(lab: Lab) -> None:
    X, hap = lab.P["end_exclude_len"], lab.P["use_haplo_ct"]
    if X:
        lab.single(T(s=(3, 0, 0, 0), i=(1, 1, 1, 0)))         # `continue` hides a passing insert
        lab.single(T(d=1, s=(2, 0, 0, 0), i=(0, 1, 1, 0)))
        if not hap:
            lab.single(T(s=(3, 4, 0, 0), i=(1, 1, 1, 0)))     # substitution and insert records
            lab.single(T(d=4, s=(3, 0, 0, 0), i=(1, 1, 1, 0)))    # delete and insert records
            lab.single(T(d=4, s=(0, 0, 3, 0), i=(0, 1, 1, 1)), own=2, nxt=0)
    else:
        lab.single(T(c=3, i=(1, 1, 1, 0)))                    # confirmed >= 2, no_insert 0
        lab.single(T(c=2, d=5, i=(1, 1, 0, 0)))
        lab.single(T(c=1, d=7, ni=1))
        lab.single(T(c=0, d=2, i=(0, 0, 0, 0)))


def _saturated(lab: Lab, tally_true) -> None:
    """single() for counts past MAX_VOTE: the pieces of the true counts, the tally held at 255."""
    lab.single(tally_true)
    a, j, t = lab.want.pop()
    lab.expect(a, j, [min(v, FR.MAX_VOTE) for v in t])


def saturation(lab: Lab, plane: str, n: int) -> None:
    """n votes on one plane (255, 256, 300 ...), next to counts that make the held value show."""
    X, hap = lab.P["end_exclude_len"], lab.P["use_haplo_ct"]
    if plane == "subst":                  # 2 * 255 <= 255 + 255 only while c is held at 255
        assert not hap
        _saturated(lab, T(s=(0, n, 255, 0)))
    elif plane == "subst_confirmed_1":    # `confirmed` at exactly 1 lets max > 6 through
        _saturated(lab, T(c=1, s=(0, n, 0, 0)))
    elif plane == "insert":               # 2 * 255 < 255 + 250 + 6 only while a is held at 255
        assert X == 0 and not hap
        _saturated(lab, T(c=n + 256, i=(n, 250, 6, 0)))
    elif plane == "insert_no_insert_1":
        assert X == 0 and not hap
        _saturated(lab, T(c=n + 301, ni=1, i=(n, 200, 100, 0)))
    elif plane == "confirmed":            # a count that wrapped at 256 would give a record
        _saturated(lab, T(c=n, s=(0, 2, 0, 0)))
    elif plane == "no_insert":
        assert X == 0
        _saturated(lab, T(c=n + 5, ni=n, i=(2, 2, 1, 0)))
    else:
        raise KeyError(plane)


def insert_flip(lab: Lab) -> None:
    """300 + 200 + 60 inserted letters: 2 * 300 >= 560 is no record, the held 2 * 255 < 515 is."""
    assert lab.P["end_exclude_len"] == 0 and not lab.P["use_haplo_ct"]
    _saturated(lab, T(c=560, i=(300, 200, 60, 0)))


POSITIONS = (254, 255, 256, 257, 511, 512)


def positions(lab: Lab) -> None:
    """k_fe_decide's blocks of 256 bases.  The first base that votes is base 0 and the last is
    the read's last base, both for substitutions from a piece that starts in A's base 0 (:282
    keeps every later start from voting at the last base); a deletion votes at base 0 as well."""
    X, hap, W = lab.P["end_exclude_len"], lab.P["use_haplo_ct"], lab.W
    two = T(s=(0, 2, 0, 0))
    for j in POSITIONS:
        a = lab.add_a(j + W + 2, {j: (0, 3)})
        lab.site(a, j, two, lo=0)
    a = lab.add_a(2 * W + 3, {0: (0, 3)})                     # the first base
    lab.site(a, 0, two, lo=0)
    a = lab.add_a(2 * W + 3, {0: (0, 3)})
    lab.site(a, 0, T(d=2), lo=0)
    lab.add_a(50)                                             # in range, no overlap
    for n in (2 * W + 3, 256, 257):                           # the last base
        a = lab.add_a(n, {n - 1: (0, 3)})
        lab.site(a, n - 1, two, lo=0)
    # `confirmed` and `no_insert` that began in another block are what refuses: pieces from
    # A's base 0, so that their counts reach the site only through the carry between blocks
    a = lab.add_a(256 + W + 2, {256: (0, 3)})
    lab.site(a, 256, T(c=2, s=(0, 2, 0, 0)), lo=0)
    a = lab.add_a(257 + W + 2, {257: (0, 3)})
    if X == 0:
        lab.site(a, 257, T(c=7, ni=2, i=(2, 2, 1, 0)), lo=0)
    elif not hap:
        lab.site(a, 257, T(c=1, s=(3, 7, 0, 0), ni=1, i=(1, 1, 1, 0)), lo=0)
    else:
        lab.site(a, 257, T(c=1, s=(0, 6, 0, 0), ni=1), lo=0)
    # records at 255 and at 256 of one read: pieces with both substitutions
    a = lab.add_a(300, {255: (0, 3)})
    hi = 256 + W + 1
    if X and not hap:                                         # and two records at 255
        lab.piece(a, 0, hi, [(255, "S", 1), (256, "S", 1)], copies=4)
        for k in range(3):
            lab.piece(a, 0, hi, [(255, "I", k)])
        lab.expect(a, 255, T(s=(3, 4, 0, 0), i=(1, 1, 1, 0)))
        lab.expect(a, 256, T(s=(0, 4, 0, 3)))
    else:
        lab.piece(a, 0, hi, [(255, "S", 1), (256, "S", 1)], copies=2)
        lab.expect(a, 255, two)
        lab.expect(a, 256, two)


def degrees(lab: Lab) -> None:
    """Reads with l overlaps on the left end and r on the right, some hanging over the end."""
    for l, r in ((1, 2), (2, 1), (2, 3), (3, 2), (13, 14)):
        a = lab.add_a(60)
        for k in range(l):
            lab.piece(a, 0, 40, lead=lab.rand(5) if k % 2 else b"")
        for k in range(r):
            lab.piece(a, 20, 60, trail=lab.rand(4) if k % 2 else b"")


def short_kmer(lab: Lab) -> None:
    """kmer_len < 2 * end_exclude_len: match runs of kmer_len, 2X - 1, 2X and 2X + 1 bases
    between two changes, next to the alignment's start and next to its end, from pieces that
    start in A's base 0 and behind it.  Every piece comes twice, so that its changes decide."""
    K, X = lab.P["kmer_len"], lab.P["end_exclude_len"]
    assert K < 2 * X
    runs = (K - 1, K, 2 * X - 1, 2 * X, 2 * X + 1)

    def sub(a, at):
        return (at, "S", (_ACGT.index(lab.a_reads[a][at]) + 1) % 4)

    for lo in (0, 7):
        for r in runs:                                        # between two changes
            a = lab.add_a(120)
            s1 = lo + 2 * X + 3
            lab.piece(a, lo, s1 + r + 1 + 2 * X + 4, [sub(a, s1), sub(a, s1 + r + 1)], copies=2)
        for r in runs:                                        # next to the alignment's start
            if lo + r - X < 0:
                continue                                      # would vote in front of the read
            a = lab.add_a(120)
            lab.piece(a, lo, lo + r + 30, [sub(a, lo + r)], copies=2)
        for r in runs:                                        # next to A's end, one base short
            a = lab.add_a(90)
            lab.piece(a, lo, 89, [sub(a, 88 - r)], copies=2)
    a = lab.add_a(120)                                        # :282: the change does not vote
    lab.piece(a, 50, 90, [sub(a, 75), (60, "D", 0)], copies=2)


def random_sites(lab: Lab, n: int) -> None:
    """n sites of random small tallies, each in an A read of its own."""
    rng, X = lab.rng, lab.P["end_exclude_len"]
    few = (0, 0, 0, 0, 1, 1, 2, 2, 3, 4, 7)
    pick = lambda: int(few[int(rng.integers(0, len(few)))])
    for _ in range(n):
        own = int(rng.integers(0, 4))
        nxt = (own + int(rng.integers(1, 4))) % 4
        s = [pick() if k != own else 0 for k in range(4)]
        ins = [min(pick(), 3) if k != nxt and rng.random() < 0.5 else 0 for k in range(4)]
        ni = int(rng.integers(0, 3)) if rng.random() < 0.5 else 0
        ends = int(rng.integers(0, 3)) if rng.random() < 0.5 else 0
        s[own] = (sum(ins) + (pick() if rng.random() < 0.3 else 0)) if X else 0
        c = ni + ends + (0 if X else sum(ins))
        lab.single(T(c=c, d=pick() if rng.random() < 0.4 else 0, s=s, ni=ni, i=ins), own, nxt)


GROUPS = {"substitution": substitution, "insert": insert, "interaction": interaction,
          "positions": positions, "degrees": degrees}


def fixture(name: str) -> Lab:
    """The job of tests/golden/fe_<name>.npz, e..i: every group under that option line."""
    lab = Lab(5200 + ord(name), LINES[name])
    for g in GROUPS.values():
        g(lab)
    if name == "i":
        insert_flip(lab)
    if name == "h":
        short_kmer(lab)
    lab.false_pair(0)
    return lab


# ------------------------------------------------------------------- the instrumented walk

def _insert_ladder(t, hap, n=None):
    """The second ladder of Output_Corrections (findErrors-Output.C:169-229) -> vote or None."""
    n = collections.Counter() if n is None else n
    NI, I0 = FR.NO_INSERT, FR.INSERT0
    four = t[I0:I0 + 4]
    ins, imx = FR.A_INSERT, four[0]
    for c in range(1, 4):
        if imx < four[c]:
            ins, imx = FR.A_INSERT + c, four[c]
    ihap = sum(v >= FR.MIN_HAPLO_OCCURS for v in four)
    itot = sum(four)
    if t[NI] >= 2:
        if imx in (6, 7):
            n[f"no_insert 2, ins_max {imx}"] += 1
        return None
    if itot in (1, 2):
        n[f"ins_total {itot}"] += 1
    if itot <= 1:
        return None
    if 2 * imx == itot:
        n["2 ins_max == ins_total"] += 1
    if 2 * imx >= itot:
        return None
    if 2 * imx == itot - 1:
        n["2 ins_max == ins_total - 1"] += 1
    if sum(v == imx for v in four) > 1:
        n["ins_max tied"] += 1
    if ihap >= 2:
        n["ins_haplo_ct >= 2, refused" if hap else "ins_haplo_ct >= 2 with -p"] += 1
        if hap:
            return None
    else:
        n["ins_haplo_ct < 2"] += 1
    if imx in (6, 7):
        n[f"no_insert {t[NI]}, ins_max {imx}"] += 1
    if t[NI] > 0 and (t[NI] != 1 or imx <= 6):
        n["no_insert 1, ins_max <= 6: refused"] += 1
        return None
    n["insert record"] += 1
    if t[NI] == 1:
        n["insert record with no_insert 1"] += 1
    if imx >= FR.MAX_VOTE:
        n["insert plane at MAX_VOTE"] += 1
    return ins


def walk(tallies, deg, reads, bgn, end, P):
    """Output_Corrections (findErrors-Output.C:59-231) with a counter on every branch
    -> (.red records, counts).  The records must equal fe_restate.output_corrections'."""
    n = collections.Counter()
    out = []
    hap, X, thr = P["use_haplo_ct"], P["end_exclude_len"], P["degree_threshold"]
    C, D, S0, NI = FR.CONFIRMED, FR.DELETES, FR.SUBST0, FR.NO_INSERT
    with_records = []
    for rid in range(bgn, end + 1):
        keep = (deg[rid][0] < thr) | ((deg[rid][1] < thr) << 1)
        out.append((keep, rid))
        for side, name in enumerate(("left", "right")):
            if deg[rid][side] in (thr - 1, thr):
                n[f"{name} degree == threshold" + (" - 1" if deg[rid][side] < thr else "")] += 1
        if max(deg[rid]) > 12:
            n["degree above 12"] += 1
        Tl = tallies[rid]
        L = Tl.shape[0]
        Sq = FR.filter_read(reads[rid])
        first = len(out)
        for j in range(L):
            t = [int(v) for v in Tl[j]]
            if not any(t[1:]):
                continue
            if max(t) > 13:
                n["tally above 13"] += 1
            five = [t[D]] + t[S0:S0 + 4]
            vote, mx, is_change = FR.DELETE, t[D], True
            for c in range(4):
                if t[S0 + c] > mx:
                    vote, mx, is_change = FR.A_SUBST + c, t[S0 + c], int(Sq[j]) != c
            haplo = sum(v >= FR.MIN_HAPLO_OCCURS for v in five)
            total = sum(five)
            sub = None
            if t[C] < 2:
                why = None
                if total in (1, 2):
                    n[f"total {total}"] += 1
                if mx and t[D] == mx and mx in t[S0:S0 + 4]:
                    n["max tied between delete and a letter"] += 1
                if mx and sum(v == mx for v in t[S0:S0 + 4]) > 1:
                    n["max tied between two letters"] += 1
                if total <= 1:
                    why = "few"
                elif 2 * mx <= total:
                    why = "weak"
                    if 2 * mx == total:
                        n["2 max == total"] += 1
                elif not is_change:
                    why = "same"
                    n["!is_change"] += 1
                    if X == 0:
                        n["!is_change with -x 0"] += 1
                elif haplo >= 2 and hap:
                    why = "haplo"
                    n["haplo_ct >= 2, refused"] += 1
                    if sorted(five)[-2] == FR.MIN_HAPLO_OCCURS:
                        n["second value at MIN_HAPLO_OCCURS, refused"] += 1
                elif t[C] > 0 and (t[C] != 1 or mx <= 6):
                    why = "indet"
                    n["confirmed 1, max <= 6: refused"] += 1
                if why is None or why == "indet":
                    if mx in (6, 7):
                        n[f"confirmed {t[C]}, max {mx}"] += 1
                if why is not None:
                    if _insert_ladder(t, hap) is not None:
                        n["substitution `continue` hides a passing insert"] += 1
                    continue
                sub = vote
                out.append((keep | (vote << 2) | (j << 6), rid))
                n["substitution record" if vote != FR.DELETE else "delete record"] += 1
                if 2 * mx == total + 1:
                    n["2 max == total + 1"] += 1
                if t[C] == 1:
                    n["record with confirmed 1"] += 1
                if haplo >= 2:
                    n["haplo_ct >= 2 with -p"] += 1
                    if sorted(five)[-2] == FR.MIN_HAPLO_OCCURS:
                        n["second value at MIN_HAPLO_OCCURS with -p"] += 1
                elif sorted(five)[-2] == FR.MIN_HAPLO_OCCURS - 1:
                    n["second value below MIN_HAPLO_OCCURS"] += 1
                if mx >= FR.MAX_VOTE:
                    n["substitution plane at MAX_VOTE"] += 1
            else:
                if mx in (6, 7):
                    n[f"confirmed 2, max {mx}"] += 1
                if j > 255 and total > 1 and 2 * mx > total and is_change:
                    n["confirmed >= 2 refuses past base 255"] += 1
            if t[C] >= FR.MAX_VOTE:
                n["confirmed at MAX_VOTE"] += 1
            ins = _insert_ladder(t, hap, n)
            if ins is None:
                if j > 255 and t[NI] and _insert_ladder(t[:NI] + [0] + t[NI + 1:], hap) is not None:
                    n["no_insert refuses past base 255"] += 1
                continue
            out.append((keep | (ins << 2) | (j << 6), rid))
            if sub is not None:
                n["two records at one base"] += 1
                if sub == FR.DELETE:
                    n["delete and insert records at one base"] += 1
                if j % 256 == 255:
                    n["two records at the last base of a block"] += 1
            elif t[NI] == 0:
                n["insert record with confirmed >= 2, no_insert 0"] += 1
        at = sorted(set(int(w) >> 6 for w, _ in out[first:]))
        for j in at:
            if j in POSITIONS or j == 0:
                n[f"record at base {j}"] += 1
            if j == L - 1:
                n["record at the last base"] += 1
                if L in (256, 257):
                    n[f"record at the last base of a read of {L}"] += 1
            if j % 256 == 255 and j + 1 in at:
                n["records on both sides of a block boundary"] += 1
        with_records.append(bool(at))
        if len(with_records) >= 3 and with_records[-3:] == [True, False, True] and \
                deg[rid - 1] == [0, 0]:
            n["a read with no overlap between two with records"] += 1
    red = np.array(out, dtype=FR.RED_DTYPE) if out else np.zeros(0, dtype=FR.RED_DTYPE)
    return red, n


# what the fixtures together must reach (tests/test_fe_cpu.py::test_fixtures_reach_every_branch)
REQUIRED = (
    # the rows of the branch table
    "insert record", "insert record with no_insert 1", "no_insert 1, ins_max <= 6: refused",
    "ins_haplo_ct >= 2, refused", "two records at one base", "haplo_ct >= 2, refused",
    "record with confirmed 1", "confirmed 1, max 6", "!is_change",
    "substitution `continue` hides a passing insert",
    # the substitution ladder
    "total 1", "total 2", "2 max == total", "2 max == total + 1",
    "max tied between delete and a letter", "max tied between two letters",
    "second value below MIN_HAPLO_OCCURS", "second value at MIN_HAPLO_OCCURS, refused",
    "second value at MIN_HAPLO_OCCURS with -p", "delete record", "substitution record",
    "confirmed 0, max 6", "confirmed 0, max 7", "confirmed 1, max 7", "confirmed 2, max 6",
    "confirmed 2, max 7",
    # the insert ladder
    "no_insert 0, ins_max 6", "no_insert 0, ins_max 7", "no_insert 1, ins_max 6",
    "no_insert 1, ins_max 7", "no_insert 2, ins_max 6", "no_insert 2, ins_max 7",
    "ins_total 1", "ins_total 2", "2 ins_max == ins_total", "2 ins_max == ins_total - 1",
    "ins_max tied", "ins_haplo_ct >= 2 with -p", "ins_haplo_ct < 2",
    # interaction
    "delete and insert records at one base", "insert record with confirmed >= 2, no_insert 0",
    # saturation and the gaps
    "insert plane at MAX_VOTE", "confirmed at MAX_VOTE", "tally above 13", "degree above 12",
    # positions
    *(f"record at base {j}" for j in (0,) + POSITIONS), "record at the last base",
    "record at the last base of a read of 256", "record at the last base of a read of 257",
    "records on both sides of a block boundary", "two records at the last base of a block",
    "confirmed >= 2 refuses past base 255", "no_insert refuses past base 255",
    "a read with no overlap between two with records",
    # degrees
    "left degree == threshold", "left degree == threshold - 1", "right degree == threshold",
    "right degree == threshold - 1",
)
