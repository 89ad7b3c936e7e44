"""The extension's per-pair state and delta plumbing (k_extend's glue around the row loops).

process_pair keeps a pair's distinct overlaps and the wave's output counters in a per-wave
LDS block, and extend_alignment merges the forward traceback's stack straight into
Left_Delta.  Every case here is bit-exact records and all -s counters against the oracle, as
test_gpu_parity._check, on a job chosen (with the oracle, on the CPU) so that the path named
in the test is taken; each test asserts that precondition itself.
"""
import numpy as np
import pytest

from canu_amd.synth import random_genome, synth_reads
from canu_amd.overlap_in_core import OicParameters, OverlapInCore

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


def _check(rs, P):
    """GPU records and counters equal to the oracle's; returns (records, GPU stats, oracle
    stats)."""
    oic = OverlapInCore(P, device=0)
    oic.load_reads(rs)
    oic.build_hash_index(1, 0xFFFFFFFF)
    n = oic.find_overlaps(1, 0xFFFFFFFF)
    got = oic.fetch(n)
    st = oic.stats()
    oic.close()
    want, wst = oracle.run_oracle(rs, P.as_dict(), with_stats=True)
    print({f: (st[f], wst[f]) for f in COUNTERS},
          {f: st.get(f) for f in ("pairs", "seed_nodes", "staged_pairs", "long_pairs",
                                  "generic_pairs", "extend_launches")})
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    for f in COUNTERS:
        assert st[f] == wst[f], (f, st[f], wst[f])
    return got, st, wst


def _records_per_read_pair(rec):
    """Records per unordered read pair (a record's a / b order depends on the hangs)."""
    lo = np.minimum(rec["a"], rec["b"]).astype(np.uint64)
    hi = np.maximum(rec["a"], rec["b"]).astype(np.uint64)
    _, cnt = np.unique((lo << np.uint64(32)) | hi, return_counts=True)
    return cnt


def _tandem_reads():
    # 2 kb reads from five tandem copies of a 1.5 kb unit (itself with short repeats): two
    # reads align on several diagonals 1.5 kb apart, each reaching the reads' ends, so a pair
    # fills up to three distinct-overlap slots; diagonals of one sign intersect (the entry is
    # widened, and replaced when the new alignment is better), those of opposite sign do not
    unit = random_genome(np.random.default_rng(4), 1500, 6, 60)
    g = np.tile(unit, 5)
    return synth_reads(60, 2000, g.shape[0], 0.02, seed=4, genome=g)


@pytest.mark.parametrize("partial", [False, True])
def test_three_overlap_slots(built, partial):
    """All three distinct-overlap slots and add_overlap's widen / replace paths, with the
    overlaps in the LDS state block; Merge_Intersecting_Olaps (or, partial, no merge) at the
    end."""
    kw = dict(Unique_Olap_Per_Pair=False)
    if partial:
        kw["Doing_Partial_Overlaps"] = True
    got, st, wst = _check(_tandem_reads(), _params(**kw))
    cnt = _records_per_read_pair(got)
    assert cnt.max() >= 2 and wst["multi_overlaps"] > 0
    if partial:
        assert cnt.max() == 3                  # every slot used and emitted


def test_many_nodes_per_pair(built):
    """Pairs with more matches than one 64-lane stride (12 kb reads at 3 % error): the
    longest-match search and the removal pass take two and three strides, over ~16
    extensions' worth of removal marks.  Two reads differ at ~6 % of an overlap's columns, so
    an exact run reaches k = 22 with probability 0.94^22 = 0.26 and a mean 6 kb overlap holds
    ~360 * 0.26 = 90-odd matches, twice that at full length: the mean over all pairs is
    asserted to be past 1.25 strides.  (16 reads: a pair's node count does not depend on the
    read count, and the oracle's time does.)"""
    rs = synth_reads(16, 12_000, 32_000, 0.03, seed=33)
    got, st, _ = _check(rs, _params(minlen=500))
    assert got.shape[0] > 20
    assert st["seed_nodes"] > 80 * st["pairs"], (st["seed_nodes"], st["pairs"])


def test_delta_plumbing_ragged(built):
    """Ragged lengths (0.4 .. 1.6 x 2.5 kb), both strands: the forward and the reverse call
    each run with either string first (S_Right_Len <= T_Right_Len and the opposite, likewise
    on the left), so Right_Delta is merged with either sign; contained and dovetail overlaps
    both occur."""
    rs = synth_reads(120, 2500, 30_000, 0.025, seed=35, len_jitter=0.6)
    got, st, wst = _check(rs, _params())
    flip = (got["w0"] >> np.uint64(54)) & np.uint64(1)
    assert 0 < int(flip.sum()) < got.shape[0]
    assert wst["contained_overlaps"] > 50 and wst["dovetail_overlaps"] > 50
    assert int(rs.lengths.max()) > 2 * int(rs.lengths.min())


def test_delta_plumbing_window_filter(built):
    """-w on ragged reads with qualities: the window filter walks each kept overlap's own copy
    of the merged Left_Delta, so a wrong delta changes which overlaps are rejected."""
    rs = synth_reads(n_reads=90, read_len=2500, genome_len=20_000, error_rate=0.015, seed=53,
                     with_quals=True, bursts=1, len_jitter=0.6)
    got, _, _ = _check(rs, _params(k=20, Use_Window_Filter=True))
    nowin = oracle.run_oracle(rs, _params(k=20).as_dict())
    assert 0 < got.shape[0] < nowin.shape[0]      # the filter did reject overlaps


def test_defer_and_restore(built):
    """maxErate 0.144 on 6-8 kb reads at 5 % error: some pairs' bands outgrow the register
    window after earlier extensions of the pair succeeded, so they leave the first staged
    class with overlaps already in the state block and nodes marked removed.  The next pair
    of that wave, and the deferred pair's rerun in a later class, must not see that state."""
    rs = synth_reads(20, 7000, 28_000, 0.05, seed=37, len_jitter=0.15)
    _, st, _ = _check(rs, _params(k=16, erate=0.144, minlen=500))
    assert st["staged_pairs"] > 0
    assert st["long_pairs"] + st["generic_pairs"] > 0, st


def test_counters(built):
    """Hopeless singletons and the --minkmers filter: kmer_hits_without_olap and
    kmer_hits_skipped (counters kept in the LDS state block) equal the oracle's."""
    rs = synth_reads(120, 2000, 30_000, 0.03, seed=39)
    P = _params(minlen=500)
    P.Filter_By_Kmer_Count = int(np.floor(np.exp(-1.0 * 22 * P.maxErate) * (500 - 22 + 1)))
    _, st, wst = _check(rs, P)
    assert wst["kmer_hits_skipped"] > 0 and wst["kmer_hits_without_olap"] > 0
    assert st["kmer_hits_skipped"] == wst["kmer_hits_skipped"]
    assert st["kmer_hits_without_olap"] == wst["kmer_hits_without_olap"]
