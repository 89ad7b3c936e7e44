"""The staged row loop's end bookkeeping (wave_ped_reg of canu_amd/csrc/ovl_extend.hip): rows
further than `row_end_margin()` bases from both reads' ends ("interior" rows) skip the
per-cell count of the bases left, and only lanes that continue past their first 31 matches
can reach an end there; rows nearer an end keep the full step.

Every case is bit-exact records and all -s counters against the oracle, on a job chosen (with
the oracle and the synthetic truth, on the CPU) so that the rows named in the test occur; each
test asserts that precondition itself.
"""
import numpy as np
import pytest

from canu_amd.synth import ReadSet, synth_reads, _COMP
from canu_amd.overlap_in_core import OicParameters, OverlapInCore, row_end_margin

import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("kmer_hits_with_olap", "kmer_hits_without_olap", "total_overlaps",
            "contained_overlaps", "dovetail_overlaps", "seed_hits", "multi_overlaps",
            "kmer_hits_skipped")
HM = np.uint64(0x1FFFFF)


def _params(**kw):
    P = OicParameters(Kmer_Len=kw.pop("k", 22), maxErate=float(np.float32(kw.pop("erate", 0.06))),
                      Min_Olap_Len=kw.pop("minlen", 100))
    for k, v in kw.items():
        setattr(P, k, v)
    return P.finalize()


def _check(rs, P, want, wst):
    """GPU records and counters equal to the oracle's (`want`, `wst`)."""
    oic = OverlapInCore(P, device=0)
    oic.load_reads(rs)
    oic.build_hash_index(1, 0xFFFFFFFF)
    n = oic.find_overlaps(1, 0xFFFFFFFF)
    got = oic.fetch(n)
    st = oic.stats()
    oic.close()
    print({f: (st[f], wst[f]) for f in COUNTERS},
          {f: st.get(f) for f in ("pairs", "staged_pairs", "long_pairs", "generic_pairs")})
    assert st["staged_pairs"] > 0                 # the register row loop ran
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    for f in COUNTERS:
        assert st[f] == wst[f], (f, st[f], wst[f])


def _fields(rec):
    """ahg5, ahg3, bhg5, bhg3, span, flipped, evalue of each record, as int64."""
    w0, w1 = rec["w0"], rec["w1"]
    i = lambda x: x.astype(np.int64)
    return (i(w0 & HM), i((w0 >> np.uint64(21)) & HM), i(w1 & HM), i((w1 >> np.uint64(21)) & HM),
            i((w1 >> np.uint64(42)) & HM), i((w0 >> np.uint64(54)) & np.uint64(1)),
            i((w0 >> np.uint64(42)) & np.uint64(0xfff)))


def _reaches_ends(rec):
    """Per record: at each end of the overlap one of the two reads has no hang."""
    a5, a3, b5, b3, _, _, _ = _fields(rec)
    return ((a5 == 0) | (b5 == 0)) & ((a3 == 0) | (b3 == 0))


def _error_counts(rec):
    _, _, _, _, span, _, ev = _fields(rec)
    return np.rint(ev * span / 10000.0).astype(np.int64)


def _genome_strand(rs, i):
    """Read i as it lies on the genome's forward strand."""
    o, L = int(rs.offsets[i]), int(rs.lengths[i])
    r = rs.bases[o:o + L]
    return _COMP[r[::-1]] if rs.strands[i] else r


def _with_bases(rs, bases):
    return ReadSet(bases=bases, offsets=rs.offsets, lengths=rs.lengths, quals=None,
                   first_iid=rs.first_iid, starts=rs.starts, strands=rs.strands)


_SUB = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


def _end_runs(rs, rec):
    """For substitution-only reads (genome coordinates are exact).  Per record that covers
    the whole true region on both reads (by its hangs): the matches left of the region's
    first mismatch and right of its last one, which read (0 = the record's a, 1 = b) ends the
    region on each side, and the number of mismatches.  Returns arrays (index into rec, left
    run, left ender, right run, right ender, mismatches)."""
    a5, a3, b5, b3, _, _, _ = _fields(rec)
    out = []
    for x in range(rec.shape[0]):
        a, b = int(rec["a"][x]) - rs.first_iid, int(rec["b"][x]) - rs.first_iid
        sa, sb = int(rs.starts[a]), int(rs.starts[b])
        ea, eb = sa + int(rs.lengths[a]), sb + int(rs.lengths[b])
        lo, hi = max(sa, sb), min(ea, eb)
        if ea - sa - int(a5[x] + a3[x]) != hi - lo or eb - sb - int(b5[x] + b3[x]) != hi - lo:
            continue
        if sa == sb or ea == eb:
            continue
        mm = np.nonzero(_genome_strand(rs, a)[lo - sa:hi - sa] !=
                        _genome_strand(rs, b)[lo - sb:hi - sb])[0]
        if mm.size == 0:
            continue
        out.append((x, int(mm[0]), 0 if sa > sb else 1, hi - lo - 1 - int(mm[-1]),
                    0 if ea < eb else 1, mm.size))
    return np.array(out, dtype=np.int64).reshape(-1, 6).T


@pytest.mark.parametrize("error", [0.01, 0.03])
def test_no_interior_row(built, error):
    """Reads of 120-300 bases: the extensions' rows are within the margin of an end almost
    from their start, so the full step alone has to give the oracle's records."""
    rs = synth_reads(100, 210, 1500, error, seed=61, len_jitter=0.42)
    assert 120 <= int(rs.lengths.min()) and int(rs.lengths.max()) <= 300
    P = _params(minlen=40)
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    assert want.shape[0] > 200 and (_error_counts(want) > 0).sum() > 50
    assert 0 < int(rs.strands.sum()) < rs.nreads
    _check(rs, P, want, wst)


def test_switch_over(built):
    """Ragged 600-2,000-base reads at 2.5 % error on both strands: extensions start on
    interior rows and finish on rows near an end."""
    M = row_end_margin()
    rs = synth_reads(100, 1300, 10_000, 0.025, seed=63, len_jitter=0.54)
    assert 590 <= int(rs.lengths.min()) and int(rs.lengths.max()) <= 2010
    assert 0 < int(rs.strands.sum()) < rs.nreads
    P = _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    _, _, _, _, span, flipped, _ = _fields(want)
    print("records", want.shape[0], "span / margin quartiles", np.percentile(span, [25, 50, 75]) / M)
    assert want.shape[0] > 300 and 0 < int(flipped.sum()) < want.shape[0]
    # each side of an overlap (from its seed to an end) is many margins long ...
    assert np.median(span) > 12 * M and (span > 30 * M).any()
    # ... with errors on the way (rows), and the overlaps reach the reads' ends
    assert (_error_counts(want) >= 4).mean() > 0.8
    assert _reaches_ends(want).all()
    _check(rs, P, want, wst)


EDGES = (30, 31, 32, 33, 34, 63, 64, 65)


def _edge_reads(n_reads, seed):
    """Error-free ragged reads with substitutions planted D, D + 97, D + 197 and D + 297
    bases from each end of read i, D = EDGES[i % 8]: the mismatch nearest an end has exactly D
    matching bases between it and the end."""
    rs = synth_reads(n_reads, 1300, 9_000, 0.0, seed=seed, len_jitter=0.5)
    bases = rs.bases.copy()
    for i in range(rs.nreads):
        o, L = int(rs.offsets[i]), int(rs.lengths[i])
        for g in (0, 97, 197, 297):
            for p in (o + EDGES[i % 8] + g, o + L - 1 - EDGES[i % 8] - g):
                bases[p] = _SUB[int(bases[p])]
    return _with_bases(rs, bases)


def test_ends_at_margin_edges(built):
    """The last mismatch before an alignment's end lies 30 .. 34 and 63 .. 65 bases from it:
    the rows where a first-step lane's bases left are exactly at, below and above what the
    interior test promises (and the second slide step's edge).  The read that ends there is
    the record's a read or its b read (so the end binds through m in one and through n in the
    other, contained overlaps included), at the region's left end (the reverse call) and at
    its right end (the forward call), on both strands."""
    M = row_end_margin()
    assert 31 < M <= 34                                           # EDGES bracket the margin
    rs = _edge_reads(104, seed=65)
    assert int(rs.lengths.min()) >= 640
    P = _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    a5, a3, b5, b3, _, flipped, _ = _fields(want)
    x, lrun, lend, rrun, rend, nmm = _end_runs(rs, want)
    assert x.size > 300 and (nmm >= 4).mean() > 0.8
    contained = ((a5 == 0) & (a3 == 0)) | ((b5 == 0) & (b3 == 0))
    print("records", want.shape[0], "checked", x.size, "contained", int(contained[x].sum()))
    for D in EDGES:
        for run, ender, side in ((lrun, lend, "left"), (rrun, rend, "right")):
            for who in (0, 1):
                hit = (run == D) & (ender == who)
                assert hit.any(), (D, side, who)
            assert 0 < flipped[x[run == D]].sum() < (run == D).sum(), (D, side)
            assert contained[x[run == D]].any(), (D, side)
    _check(rs, P, want, wst)


def test_large_hangs(built):
    """Dovetails whose hang is most of a read's length, in both signs, and contained
    overlaps: the extensions start next to a read's end, run the other way through interior
    rows, and the cells outside the band carry large diagonals."""
    rs = synth_reads(110, 2000, 14_000, 0.02, seed=67, len_jitter=0.45)
    P = _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    a5, a3, b5, b3, span, flipped, _ = _fields(want)
    La = rs.lengths[want["a"].astype(np.int64) - rs.first_iid].astype(np.int64)
    Lb = rs.lengths[want["b"].astype(np.int64) - rs.first_iid].astype(np.int64)
    print("records", want.shape[0], "max hang share", (a5 / La).max(), (b5 / Lb).max(),
          (a3 / La).max(), (b3 / Lb).max())
    # the a read hangs out on the left (positive a hang) / the b read does (negative)
    assert ((a5 > 0.8 * La) & (a5 > 900)).sum() >= 5
    assert ((b5 > 0.8 * Lb) & (b5 > 900)).sum() >= 5
    assert ((a3 > 0.8 * La) & (a3 > 900)).sum() >= 5
    assert ((b3 > 0.8 * Lb) & (b3 > 900)).sum() >= 5
    assert (((a5 == 0) & (a3 == 0)) | ((b5 == 0) & (b3 == 0))).sum() >= 20
    assert 0 < int(flipped.sum()) < want.shape[0]
    _check(rs, P, want, wst)


@pytest.mark.parametrize("kind", ["indels", "substitutions"])
def test_long_exact_runs(built, kind):
    """Reads at 0.4 % error: the rows' steps are hundreds of bases, so most rows have lanes
    that continue past 31 matches, and most alignments reach their end by such a run from an
    interior row (the end ballot inside the continue path).  With substitutions only the
    truth gives each end's run exactly."""
    M = row_end_margin()
    if kind == "indels":
        rs = synth_reads(100, 1500, 11_000, 0.004, seed=69, len_jitter=0.4)
    else:
        rs = synth_reads(100, 1500, 11_000, 0.004, seed=71, len_jitter=0.4, sub_frac=1.0,
                         ins_frac=0.0)
    P = _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    _, _, _, _, span, _, _ = _fields(want)
    errs = _error_counts(want)
    assert want.shape[0] > 300 and _reaches_ends(want).all()
    # errors (rows) in most overlaps, on average many margins apart
    assert (errs >= 1).mean() > 0.8
    assert np.median(span[errs >= 1] / errs[errs >= 1]) > 3 * M
    if kind == "substitutions":
        x, lrun, lend, rrun, rend, nmm = _end_runs(rs, want)
        print("checked", x.size, "end runs beyond two steps", int((lrun > 2 * M).sum()),
              int((rrun > 2 * M).sum()))
        assert x.size > 200
        # ends reached by a run that leaves the first step, from a row that is interior
        assert (lrun > 2 * M).sum() > 100 and (rrun > 2 * M).sum() > 100
        # ... and a few that end inside the margin, for contrast
        assert (lrun < M).any() and (rrun < M).any()
    _check(rs, P, want, wst)


def _junk_tails(n_reads, seed):
    """Reads at 1.5 % error; every third read's last 35 % is replaced by random bases, so an
    overlap that would run into that tail is followed by unrelated sequence."""
    rs = synth_reads(n_reads, 1600, 11_000, 0.015, seed=seed, len_jitter=0.3)
    bases = rs.bases.copy()
    rng = np.random.default_rng(seed + 1)
    junk = np.zeros(rs.nreads, dtype=np.int64)
    for i in range(0, rs.nreads, 3):
        o, L = int(rs.offsets[i]), int(rs.lengths[i])
        junk[i] = int(0.35 * L)
        bases[o + L - junk[i]:o + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[
            rng.integers(0, 4, size=junk[i])]
    return _with_bases(rs, bases), junk


@pytest.mark.parametrize("partial", [False, True])
def test_extension_stops_short(built, partial):
    """Extensions that run into unrelated sequence far from both ends: the row loop runs on
    interior rows to the error limit, or until its band is empty, and returns the max-score
    result.  Without partial overlaps the oracle counts such pairs as k-mer hits without an
    overlap; with them it reports the overlap up to the junk."""
    M = row_end_margin()
    rs, junk = _junk_tails(99, seed=73)
    # from the truth: pairs whose genome ranges share >= 400 bases of which one read's junk
    # tail covers >= 150, the tail starting >= 150 bases inside the range
    s = rs.starts
    e = s + rs.lengths.astype(np.int64)
    # the junk tail's genome range: the read's last bases lie at its genome-left end when
    # it is reverse-complemented
    jlo = np.where(rs.strands == 1, s, e - junk)
    jhi = np.where(rs.strands == 1, s + junk, e)
    hit = set()
    for i in np.nonzero(junk)[0]:
        for j in range(rs.nreads):
            lo, hi = max(s[i], s[j]), min(e[i], e[j])
            if j == i or hi - lo < 400:
                continue
            c = min(hi, jhi[i]) - max(lo, jlo[i])
            if c >= 150 and (hi - lo) - c >= 150:
                hit.add((min(i, j) + rs.first_iid, max(i, j) + rs.first_iid))
    assert len(hit) >= 30
    assert int(junk[junk > 0].min()) > 8 * M
    P = _params(Doing_Partial_Overlaps=True) if partial else _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    pairs = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in zip(want["a"], want["b"])}
    print("truth pairs", len(hit), "reported", len(hit & pairs), "records", want.shape[0],
          "without olap", wst["kmer_hits_without_olap"])
    if partial:
        # reported, and stopping short of the reads' ends on one side at least
        assert len(hit & pairs) >= 20
        a5, a3, b5, b3, _, _, _ = _fields(want)
        short = ((a5 > M) & (b5 > M)) | ((a3 > M) & (b3 > M))
        assert short.sum() >= 20
    else:
        assert wst["kmer_hits_without_olap"] >= 20
    assert want.shape[0] > 100
    _check(rs, P, want, wst)
