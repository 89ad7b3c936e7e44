"""The seams of one search (find_impl, canu_amd/csrc/ovl_find.hip) at small shapes.

A search is a loop of probe batch -> chain chunk -> accumulator -> extension launch -> output
buffer, and at every arrow indices are rebased and buffers reused: take_within cuts the units to
the window budget and then to the hit budget (the tail is probed again), plan_chain builds the
live list and the capacities, probe_sorted_run hands the chain a slice of a sorted run,
acc_append / k_append_pairs rebase unit and node indices and carry the accumulator's contents
over when it grows, flush_acc can run in the middle of a job, ensure_out moves the records held
into a bigger buffer, and the chain's out-of-memory path halves the hit budget and plans again.
Every budget behind these seams is sized for full-size jobs (3.5 G hits, 512 M windows, 4 M
pairs, 1 M records), so the parity tests' jobs make exactly one probe batch, one chain chunk and
one flush.  The OVL_TEST_* knobs (FindRun::begin) lower the budgets; ovl_stats' chain_launches,
acc_flushes, out_regrows and budget_halvings prove that the path a case names ran.

Every case compares the records with the oracle's (np.array_equal after the usual sort) and the
counters of COUNTERS.  Reference semantics: Process_Overlaps.C:101-137 over Find_Overlaps.C:
284-370 and Process_String_Olaps -- a query's overlaps do not depend on which other queries
share its batch, so every cut gives the uncut job's records.

Oracle figures behind the path assertions (if a generator change moves them, change the
budgets, not the assertions):
  A  300 units, 593,700 windows, 650,686 seed hits, 1,553 pairs, 1,495 records
  B  606,446 windows, longest unit 3,144 windows, 496,439 hits, 1,917 pairs
  C  62.4 M hits, 225,222 pairs, 11,684 records (the oracle takes ~25 s: run once)
  T  48 units, 43,300 hits, 147 pairs, 137 records
"""
import functools

import numpy as np
import pytest

from canu_amd.synth import synth_reads
from canu_amd.overlap_in_core import OicParameters, OverlapInCore

import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("seed_hits", "pairs", "kmer_hits_with_olap", "kmer_hits_without_olap",
            "kmer_hits_skipped", "multi_overlaps", "total_overlaps", "contained_overlaps",
            "dovetail_overlaps")
SEAMS = ("chain_launches", "acc_flushes", "out_regrows", "budget_halvings", "probe_launches")
KNOBS = ("OVL_TEST_HIT_BUDGET", "OVL_TEST_WIN_BUDGET", "OVL_TEST_ACC_PAIRS",
         "OVL_TEST_OUT_RECORDS", "OVL_TEST_CHAIN_ALLOC_FAILS", "OVL_TEST_PAIRS_PER_UNIT",
         "OVL_HIT_BUDGET_M")


def _concat(a, b):
    from canu_amd.synth import ReadSet
    off_b = b.offsets.astype(np.uint64) + np.uint64(a.bases.shape[0])
    return ReadSet(bases=np.concatenate([a.bases, b.bases]),
                   offsets=np.concatenate([a.offsets.astype(np.uint64), off_b]),
                   lengths=np.concatenate([a.lengths, b.lengths]).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def _reads(name):
    if name == "A":
        return synth_reads(150, 2000, 30_000, 0.02, seed=1)
    if name == "B":
        return synth_reads(150, 2000, 30_000, 0.02, seed=5, n_rate=0.002, n_repeats=6,
                           repeat_len=300, len_jitter=0.6)
    if name == "C":
        return synth_reads(700, 1000, 70_000, 0.02, seed=41, n_repeats=150, repeat_len=300)
    if name == "T":
        return synth_reads(24, 1500, 6_000, 0.02, seed=3)
    if name == "A+U":       # A, then 150 reads of an unrelated genome (hashed: A's reads only)
        return _concat(_reads("A"), synth_reads(150, 2000, 30_000, 0.02, seed=1001))
    raise KeyError(name)


def _skip_kmers(rs):
    # as test_gpu_parity.test_skip_kmers builds them: every 10th 22-mer of the first read
    r0 = rs.read(0)
    skip = [r0[i:i + 22].decode() for i in range(0, 1900, 10)]
    return tuple(s for s in skip if len(s) == 22 and set(s) <= set("ACGT"))


# name -> (read set, OicParameters keywords, skip k-mers?, hash range)
JOBS = {
    "A": ("A", {}, False, None),
    "A-partial": ("A", {"Doing_Partial_Overlaps": True}, False, None),
    "A-multi": ("A", {"Unique_Olap_Per_Pair": False}, False, None),
    "A-k16": ("A", {"k": 16}, False, None),
    "A-l3": ("A", {"Frag_Olap_Limit": 3}, False, None),
    "B-skip": ("B", {}, True, None),
    "B": ("B", {}, False, None),
    "C": ("C", {"minlen": 200}, False, None),
    "T": ("T", {}, False, None),
    "A+U": ("A+U", {}, False, (1, 150)),
}


def _params(**kw):
    P = OicParameters(Kmer_Len=kw.pop("k", 22), maxErate=float(np.float32(0.06)),
                      Min_Olap_Len=kw.pop("minlen", 100))
    for k, v in kw.items():
        setattr(P, k, v)
    return P.finalize()


def _job(name):
    rsn, kw, skip, hash_range = JOBS[name]
    rs = _reads(rsn)
    return rs, _params(**kw), (list(_skip_kmers(rs)) if skip else None), hash_range


@functools.lru_cache(maxsize=None)
def _want(name):
    """The oracle's records and counters of a job: computed once per module, never written to."""
    rs, P, skip, hash_range = _job(name)
    want, wst = oracle.run_oracle(rs, P.as_dict(), hash_range=hash_range, skip_kmers=skip,
                                  with_stats=True)
    want.setflags(write=False)
    return want, wst


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _search(name, monkeypatch, **knobs):
    """One search of job `name` under the given OVL_TEST_* knobs (HIT_BUDGET=... sets
    OVL_TEST_HIT_BUDGET): records and counters equal the oracle's; returns the stats."""
    for k, v in knobs.items():
        monkeypatch.setenv("OVL_TEST_" + k, str(v))
    rs, P, skip, hash_range = _job(name)
    oic = OverlapInCore(P, device=0)
    try:
        oic.load_reads(rs)
        if skip:
            oic.set_skip_kmers(skip)
        oic.build_hash_index(*(hash_range or (1, 0xFFFFFFFF)))
        got = oic.fetch(oic.find_overlaps(1, 0xFFFFFFFF))
        st = oic.stats()
    finally:
        oic.close()
    print("seams", name, knobs, {f: st[f] for f in SEAMS},
          {f: st[f] for f in ("extend_launches", "multi_pass_units", "chain_retries")})
    _compare(got, st, *_want(name))
    return st


def _compare(got, st, want, wst):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    for f in COUNTERS:
        assert st[f] == wst[f], (f, st[f], wst[f])


@pytest.mark.parametrize("job", ["A", "A-partial", "A-multi", "B-skip", "A-k16"])
def test_hit_budget_chunks(built, monkeypatch, job):
    """1. The probed batch is chained in hit-budget chunks (nc < nb, u0 += nc) and the tail is
    probed again: 650,686 hits under a budget of 100,000."""
    st = _search(job, monkeypatch, HIT_BUDGET=100000)
    assert st["chain_launches"] >= 5
    assert st["probe_launches"] >= st["chain_launches"]


def test_unit_over_the_budget_goes_alone(built, monkeypatch):
    """2. A hit budget of 1: every unit with hits is larger than the budget and is chained
    alone (units without hits ride along with the next one)."""
    st = _search("T", monkeypatch, HIT_BUDGET=1)
    assert 40 <= st["chain_launches"] <= 48


def test_window_budget_batches(built, monkeypatch):
    """3a. The units are probed in window-budget batches: 593,700 windows under 100,000."""
    st = _search("A", monkeypatch, WIN_BUDGET=100000)
    assert st["probe_launches"] >= 5


def test_window_budget_below_the_longest_unit(built, monkeypatch):
    """3b. A window budget of 2,000, below the longest unit's 3,144 windows: that unit is
    probed alone."""
    st = _search("B", monkeypatch, WIN_BUDGET=2000)
    assert st["probe_launches"] >= 150


def test_both_cuts_out_of_step(built, monkeypatch):
    """4. The window cut and the hit cut fall at different units."""
    st = _search("A", monkeypatch, HIT_BUDGET=70001, WIN_BUDGET=90001)
    assert st["chain_launches"] >= 5 and st["probe_launches"] >= st["chain_launches"]


def test_units_without_hits(built, monkeypatch):
    """5. The live list a strict subset: the second half's reads come from another genome and
    are not hashed, so their units have no hits (but for chance k-mers)."""
    st = _search("A+U", monkeypatch, HIT_BUDGET=100000)
    assert st["chain_launches"] >= 5


def test_accumulator_flushed_mid_job(built, monkeypatch):
    """6a. The accumulator is extended in the middle of the job, several times."""
    st = _search("A", monkeypatch, HIT_BUDGET=100000, ACC_PAIRS=200)
    assert st["acc_flushes"] >= 3
    assert st["extend_launches"] >= st["acc_flushes"]


def test_accumulator_regrows_with_contents(built, monkeypatch):
    """6b. Many chunks into one flush: the accumulator grows while it holds earlier chunks'
    units, nodes and pairs, which are carried over."""
    st = _search("A", monkeypatch, HIT_BUDGET=30000)
    assert st["acc_flushes"] == 1
    assert st["chain_launches"] >= 15


def test_accumulator_flushed_per_chunk(built, monkeypatch):
    """6c. A flush threshold of 1: every chunk with pairs is extended as it arrives."""
    st = _search("A", monkeypatch, HIT_BUDGET=100000, ACC_PAIRS=1)
    # a chunk is flushed iff it brings a pair, so there are at most as many flushes as chunks;
    # and a lower threshold never flushes less often than 6a's 200 pairs do (>= 3)
    assert st["chain_launches"] >= 5
    assert 3 <= st["acc_flushes"] <= st["chain_launches"]
    assert st["extend_launches"] >= st["acc_flushes"]


def test_output_grows_with_records_held(built, monkeypatch):
    """7. The output buffer starts at 64 records and is moved while it holds records."""
    st = _search("A", monkeypatch, HIT_BUDGET=100000, ACC_PAIRS=200, OUT_RECORDS=64)
    assert st["out_regrows"] >= 2


def test_olap_limit_chunk_by_chunk(built, monkeypatch):
    """8. -l 3: every chunk is extended from the search buffers, in the reference's per-unit
    order; the accumulator is not used."""
    st = _search("A-l3", monkeypatch, HIT_BUDGET=100000)
    assert st["chain_launches"] >= 5
    assert st["acc_flushes"] == 0


@pytest.mark.parametrize("force_regrow", [False, True])
def test_multi_pass_units_across_chunks(built, monkeypatch, force_regrow):
    """9. Units of several passes of the chain's target table (the done-set launch) in every
    one of >= 7 chunks; with 4 pairs per unit allowed at first, chunks are chained again with
    the capacity their counters ask for."""
    knobs = {"PAIRS_PER_UNIT": 4} if force_regrow else {}
    st = _search("C", monkeypatch, HIT_BUDGET=8000000, **knobs)
    assert st["chain_launches"] >= 7
    assert st["multi_pass_units"] > 100
    if force_regrow:
        assert st["chain_retries"] > 0


@functools.lru_cache(maxsize=None)
def _driver_want():
    import test_gpu_sorted_guard as G
    rs = G._reads()
    want, wst, batches = oracle.run_oracle_driver(rs, G._params(), ref_range=(1, 240), threads=4,
                                                  hashstrings=45, with_stats=True)
    want.setflags(write=False)
    return rs, want, wst, batches


@pytest.mark.parametrize("variant", ["chunks", "acc+out", "super-batches+acc+out"])
def test_chunks_inside_a_sorted_run(built, monkeypatch, variant):
    """10. A driver job over sorted query windows (test_gpu_sorted_guard's): a run is probed
    once and chained in hit-budget chunks (rbase, uh and uflags offset by u0 - R.u0).  With a
    flush threshold of 300 pairs and 64 records of room, the chunks meet mid-job flushes and
    an output buffer that is moved while it holds records.  The job's 6 hash batches fit one
    super-batch, so the third variant caps the super-batches' windows (as test_gpu_sorted_guard
    does): the driver then appends across >= 3 searches with flush=false, each starting with
    the accumulator and the output buffer as the one before left them."""
    import test_gpu_sorted_guard as G
    monkeypatch.setenv("OVL_SQ", "1")
    monkeypatch.setenv("OVL_TEST_HIT_BUDGET", "200000")
    if variant != "chunks":
        monkeypatch.setenv("OVL_TEST_ACC_PAIRS", "300")
        monkeypatch.setenv("OVL_TEST_OUT_RECORDS", "64")
    if variant == "super-batches+acc+out":
        monkeypatch.setenv("OVL_SB_WINDOWS", "250000")
    rs, want, wst, batches = _driver_want()
    oic = OverlapInCore(G._opts(G._params(), (1, 240)), device=0)
    try:
        got = oic.run_driver(rs)
        st = oic.stats()
    finally:
        oic.close()
    print("seams driver", variant, {f: st[f] for f in SEAMS},
          {f: st[f] for f in ("probe_sorted_launches", "hash_batches", "super_batches",
                              "extend_launches")})
    assert st["chain_launches"] > st["probe_sorted_launches"] > 0
    assert st["hash_batches"] == len(batches)
    if variant != "chunks":
        # thousands of pairs against a threshold of 300; the second flush finds the first's records
        assert st["acc_flushes"] >= 2 and st["out_regrows"] >= 1
    if variant == "super-batches+acc+out":
        assert 3 <= st["super_batches"] < len(batches)
    _compare(got, st, want, wst)


@pytest.mark.parametrize("job", ["A", "A+U"])
@pytest.mark.parametrize("fails", [1, 2])
def test_budget_halved_after_failed_chain_allocation(built, monkeypatch, fails, job):
    """11. The chain buffers "do not fit": the hit budget is halved, the batch planned again
    and the new plan's live list uploaded (with A+U a strict subset of the units) -- no unit
    is chained twice (seed_hits, pairs) and none is skipped."""
    st = _search(job, monkeypatch, CHAIN_ALLOC_FAILS=fails)
    assert st["budget_halvings"] == fails
    assert st["chain_launches"] >= 2


def test_knobs_unset(built, monkeypatch):
    """12. No knob: one probe batch, one chain chunk, one flush, nothing regrown or halved."""
    st = _search("A", monkeypatch)
    assert st["chain_launches"] == 1
    assert st["acc_flushes"] == 1
    assert st["out_regrows"] == 0
    assert st["budget_halvings"] == 0
    assert st["probe_launches"] == 1
