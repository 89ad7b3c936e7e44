"""The staged extension's traceback (ped_traceback_win of canu_amd/csrc/ovl_extend.hip): a
function of its own that walks the row log in windows of `traceback_window_rows()` rows.

Every case is bit-exact records and all -s counters against the oracle, on a job chosen (with
the oracle and the synthetic truth, on the CPU) so that the path named in the test is taken;
each test asserts that precondition itself.
"""
import numpy as np
import pytest

from canu_amd.synth import ReadSet, synth_reads
from canu_amd.overlap_in_core import OicParameters, OverlapInCore, traceback_window_rows

import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("kmer_hits_with_olap", "kmer_hits_without_olap", "total_overlaps",
            "contained_overlaps", "dovetail_overlaps", "seed_hits", "multi_overlaps",
            "kmer_hits_skipped")


def _params(**kw):
    P = OicParameters(Kmer_Len=kw.pop("k", 22), maxErate=float(np.float32(kw.pop("erate", 0.06))),
                      Min_Olap_Len=kw.pop("minlen", 100))
    for k, v in kw.items():
        setattr(P, k, v)
    return P.finalize()


def _check(rs, P, want=None, wst=None):
    """GPU records and counters equal to the oracle's; returns (records, GPU stats, oracle
    stats).  `want` / `wst`: the oracle's result when the test already has it."""
    oic = OverlapInCore(P, device=0)
    oic.load_reads(rs)
    oic.build_hash_index(1, 0xFFFFFFFF)
    n = oic.find_overlaps(1, 0xFFFFFFFF)
    got = oic.fetch(n)
    st = oic.stats()
    oic.close()
    if want is None:
        want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    print({f: (st[f], wst[f]) for f in COUNTERS},
          {f: st.get(f) for f in ("pairs", "seed_nodes", "staged_pairs", "long_pairs",
                                  "generic_pairs", "extend_launches")})
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    for f in COUNTERS:
        assert st[f] == wst[f], (f, st[f], wst[f])
    return got, st, wst


def _evalue(rec):
    return ((rec["w0"] >> np.uint64(42)) & np.uint64(0xfff)).astype(np.int64)


def _error_counts(rec):
    """Errors of each overlap: its error rate (evalue, 1e-4 units) times its length (span)."""
    span = ((rec["w1"] >> np.uint64(42)) & np.uint64(0x1fffff)).astype(np.int64)
    return np.rint(_evalue(rec) * span / 10000.0).astype(np.int64)


def test_window_edges(built):
    """Walks of one, two and many windows and walks that end mid-window: ragged 1.5-2.5 kb
    reads at 2.5 % error on both strands give overlaps from a few errors to several windows'
    worth.  (An extension's walk has as many rows as its side of the overlap has errors, so
    the overlaps' error counts bracket the walks' lengths from above.)"""
    R = traceback_window_rows()
    rs = synth_reads(100, 2000, 16_000, 0.025, seed=41, len_jitter=0.25)
    P = _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    errs = _error_counts(want)
    print("R", R, "error counts", np.bincount(np.minimum(errs // max(R // 2, 1), 12)))
    assert (errs < R).any() and (errs > 3 * R).any()
    assert (np.abs(errs - R) <= 1).any() and (np.abs(errs - 2 * R) <= 1).any()
    assert 0 < int(rs.strands.sum()) < rs.nreads
    assert int(rs.lengths.max()) > 1.4 * int(rs.lengths.min())
    _check(rs, P, want, wst)


def test_exact_match_no_traceback(built):
    """Error-free reads: both row-loop calls of every extension return the exact match
    (nd = -1) and no traceback runs."""
    rs = synth_reads(80, 2000, 16_000, 0.0, seed=43, len_jitter=0.3)
    P = _params()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    assert want.shape[0] > 100 and not _evalue(want).any()
    _check(rs, P, want, wst)


def _left_end_errors(n_reads, seed):
    """Error-free reads whose genome-left 200 bases carry a substitution every 50 bases.  In
    genome coordinates an overlap's region starts at the later of the two reads' starts, so
    every substitution inside it lies within its first 200 bases; with overlaps of 600 bases
    or more the longest exact match lies right of them: the extension towards the region's
    right end is an exact match (no traceback), the other one is not."""
    rs = synth_reads(n_reads, 2000, 16_000, 0.0, seed=seed, len_jitter=0.2)
    bases = rs.bases.copy()
    sub = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
    for i in range(rs.nreads):
        o, L = int(rs.offsets[i]), int(rs.lengths[i])
        for g in range(5, 200, 50):              # offset from the read's genome-left end
            p = o + (L - 1 - g if rs.strands[i] else g)
            bases[p] = sub[int(bases[p])]
    return ReadSet(bases=bases, offsets=rs.offsets, lengths=rs.lengths, quals=None,
                   first_iid=rs.first_iid, starts=rs.starts, strands=rs.strands)


def test_one_side_exact(built):
    """Only one of an extension's two row-loop calls returns the exact match: one traceback
    per extension, the other skipped."""
    rs = _left_end_errors(80, seed=45)
    P = _params(minlen=600)
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    assert want.shape[0] > 100
    # every overlap covers substitutions (its left end holds the later read's first 200
    # bases), and all of them lie in the first 200 bases of a region of >= 600
    assert _evalue(want).all()
    a = want["a"].astype(np.int64) - rs.first_iid
    b = want["b"].astype(np.int64) - rs.first_iid
    lo = np.maximum(rs.starts[a], rs.starts[b])
    hi = np.minimum(rs.starts[a] + rs.lengths[a].astype(np.int64),
                    rs.starts[b] + rs.lengths[b].astype(np.int64))
    assert (hi - lo >= 600).all()
    for r in (a, b):                             # a read's substitutions inside the region
        assert (np.maximum(rs.starts[r] + 200, lo) <= lo + 200).all()
    _check(rs, P, want, wst)


def test_cells_32bit(built):
    """Reads of 16,384 bases or more run the 32-bit-cell instances: their traceback reads
    4-byte cells from 2 KiB row stripes.  (Seven reads: the oracle's time.)"""
    rs = synth_reads(7, 17_500, 36_000, 0.02, seed=47, len_jitter=0.02)
    assert int(rs.lengths.min()) >= 16_384
    got, st, _ = _check(rs, _params(minlen=500))
    assert got.shape[0] >= 4
    assert (_error_counts(got) > 3 * traceback_window_rows()).any()


def test_wide_class_and_deferral(built):
    """maxErate 0.144 on 6-8 kb reads at 5 % error: pairs whose band outgrows the 512-wide
    register window are deferred to the 1024-wide instance, whose traceback walks 1024-cell
    row stripes (the recipe of test_gpu_extend_state.test_defer_and_restore)."""
    rs = synth_reads(20, 7000, 28_000, 0.05, seed=37, len_jitter=0.15)
    _, st, _ = _check(rs, _params(k=16, erate=0.144, minlen=500))
    assert st["staged_pairs"] > 0
    assert st["long_pairs"] + st["generic_pairs"] > 0, st


@pytest.mark.parametrize("partial", [False, True])
def test_deltas_with_other_readers(built, partial):
    """-w (and partial overlaps) on ragged reads with qualities: the window filter walks the
    merged Left_Delta, forward traceback's deltas included, so a wrong or missing delta
    changes which overlaps are rejected."""
    rs = synth_reads(n_reads=90, read_len=2500, genome_len=20_000, error_rate=0.015, seed=53,
                     with_quals=True, bursts=1, len_jitter=0.6)
    kw = dict(k=20, Doing_Partial_Overlaps=True) if partial else dict(k=20)
    got, _, _ = _check(rs, _params(Use_Window_Filter=True, **kw))
    nowin = oracle.run_oracle(rs, _params(**kw).as_dict())
    assert 0 < got.shape[0] < nowin.shape[0]      # the filter rejected some, not all
