"""The k-mer count on the device against the reference's golden texts and the numpy
restatement (tests/meryl_numpy.py, itself pinned to the golden texts by test_meryl_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import meryl_numpy as MN
from canu_amd import meryl
from canu_amd.synth import ReadSet, synth_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _count(rs, k, canonical=True, low=2, budget=None):
    mc = meryl.MerCounter(k, canonical, low, hbm_budget=budget)
    mc.load_reads(rs)
    mc.count()
    return mc


def _same(mc, want):
    st = mc.stats()
    assert (st["total_mers"], st["distinct_mers"], st["unique_mers"], st["largest_count"]) == \
        (want.total, want.distinct, want.unique, want.largest)
    assert np.array_equal(mc.histogram(), want.hist)
    for t in (0, 3):
        gm, gc = mc.frequent(t)
        wm, wc = want.frequent(t)
        assert gm.dtype == np.uint64 and gc.dtype == np.uint32
        assert np.array_equal(gm, wm) and np.array_equal(gc, wc)
    return st


@pytest.mark.parametrize("name", MN.FIXTURES)
def test_gpu_meryl_golden(built, name, tmp_path):
    """Fixtures a.-d.: totals, histogram and kept list equal the numpy values; the three texts
    are the reference's bytes, from the counting context and from the saved database."""
    rs, k, texts, want = MN.golden(name)
    mc = _count(rs, k)
    _same(mc, want)
    p = str(tmp_path / "asm")
    mc.save(p)
    for c in (mc, meryl.MerCounter.open(p)):
        c.write_histogram(p + ".h", p + ".i")
        assert open(p + ".h", "rb").read() == texts["histogram"]
        assert open(p + ".i", "rb").read() == texts["info"]
        for t, ref in texts["dt"].items():
            if t >= 2:
                c.write_threshold(t, p + ".dt")
                assert open(p + ".dt", "rb").read() == ref
        c.close()


def test_gpu_meryl_low_count_one_is_the_reference_dump(built, tmp_path):
    """Kept from count 1 on (what the reference's build does whatever its -L), -n 1 matches."""
    rs, k, texts, want = MN.golden("a_k16")
    mc = _count(rs, k, low=1)
    _same(mc, want.with_low(1))
    mc.write_threshold(1, str(tmp_path / "dt"))
    assert open(tmp_path / "dt", "rb").read() == texts["dt"][1]
    mc.close()


def test_gpu_meryl_oversize_buckets(built):
    """Fixture c (homopolymers, dinucleotide repeats): the fine buckets that exceed the LDS
    sort are split, not truncated -- and the input does reach that path."""
    rs, k, _, want = MN.golden("c_k16")
    mc = _count(rs, k)
    st = _same(mc, want)
    assert st["oversize_buckets"] > 0
    mc.close()
    # with the smallest budget the planner meets single keys larger than a pass
    mc = _count(rs, k, budget=meryl.MIN_BUDGET_BYTES)
    st = _same(mc, want)
    assert st["direct_keys"] > 0
    mc.close()
    # an oversize bucket of many different keys: 40,000 reads of exactly k bases that share
    # their first 14, so every mer falls into one bucket and differs in its low 16 bits
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = np.empty((40_000, 22), dtype=np.uint8)
    reads[:, :14] = np.frombuffer(b"GATTACAGATTACA", dtype=np.uint8)
    reads[:, 14:] = acgt[rng.integers(0, 4, (40_000, 8))]
    many = ReadSet(bases=reads.reshape(-1), offsets=np.arange(40_000, dtype=np.uint64) * 22,
                   lengths=np.full(40_000, 22, dtype=np.uint32))
    mc = _count(many, 22, canonical=False, low=1)
    st = _same(mc, MN.count_reads(many, 22, False, 1))
    assert st["oversize_buckets"] > 0 and st["distinct_mers"] > 16384
    mc.close()


@pytest.mark.parametrize("name,dense,cap", [("b_k22", 8, 1024), ("b_k22", 16, 256),
                                            ("c_k16", 65536, 4096)])
def test_gpu_meryl_overflow_list_is_drained(built, name, dense, cap):
    """Counts beyond the dense device histogram go through a short list that the host drains
    after every pass: with the dense length cut to 8 far more counts take that route than the
    list holds at once, and nothing is lost or refused.  (No mer of fixture b exceeds a pass,
    so none is counted by the planner instead.)  With the default lengths fixture c's
    homopolymer count of 199,400 takes the same route."""
    rs, k, _, want = MN.golden(name)
    mc = meryl.MerCounter(k)
    mc.set_histogram_limits(dense, cap)
    mc.load_reads(rs)
    mc.count()
    st = _same(mc, want)
    assert st["overflow_counts"] == int(want.hist[dense:].sum()) > 0
    assert st["direct_keys"] == 0
    if dense < 65536:
        assert st["overflow_counts"] > 4 * cap and st["passes"] > 4
    mc.close()
    with pytest.raises(meryl.MerError):
        meryl.MerCounter(k).set_histogram_limits(8, 8)


@pytest.mark.parametrize("min_passes", [2, 7])
def test_gpu_meryl_passes(built, min_passes):
    """Fixture b under a forced budget: several passes, the same result, and the peak within
    budget + packed reads + the fixed overhead the header states."""
    rs, k, _, want = MN.golden("b_k22")
    budget = want.total * 24 // min_passes
    mc = _count(rs, k, budget=budget)
    st = _same(mc, want)
    assert st["passes"] >= min_passes
    assert st["budget_bytes"] <= budget
    assert st["peak_device_bytes"] <= budget + st["packed_read_bytes"] + meryl.FIXED_OVERHEAD_BYTES
    one = _count(rs, k)
    assert one.stats()["passes"] == 1
    for a, b in zip(mc.frequent(0), one.frequent(0)):
        assert np.array_equal(a, b)
    assert np.array_equal(mc.histogram(), one.histogram())
    mc.close()
    one.close()


def test_gpu_meryl_deterministic_and_device_load(built):
    import torch
    rs, k, _, want = MN.golden("b_k22")
    a = _count(rs, k)
    b = _count(rs, k)
    for x, y in zip(a.frequent(0), b.frequent(0)):
        assert np.array_equal(x, y)
    # the same reads from device buffers, at offsets that are not the packed ones
    pad = 5
    offs = (rs.offsets + np.arange(rs.nreads, dtype=np.uint64) * np.uint64(pad)).astype(np.uint64)
    raw = np.full(int(offs[-1]) + int(rs.lengths[-1]) + pad, ord("N"), dtype=np.uint8)
    for i in range(rs.nreads):
        o, n = int(rs.offsets[i]), int(rs.lengths[i])
        raw[int(offs[i]):int(offs[i]) + n] = rs.bases[o:o + n]
    d_b = torch.from_numpy(raw).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    c = meryl.MerCounter(k)
    c.load_reads_device(d_b.data_ptr(), d_o.data_ptr(), rs.lengths)
    c.count()
    _same(c, want)
    for m in (a, b, c):
        m.close()


_SWEEP = [(k, canon, low, seed) for seed, (k, canon, low) in enumerate(
    [(5, True, 1), (5, False, 2), (11, True, 2), (11, False, 5), (16, True, 5), (16, False, 1),
     (22, True, 2), (22, False, 1), (27, True, 1), (27, False, 5), (32, True, 2),
     (32, False, 2)])]


def _ragged(seed):
    """50-400 reads of 0-3 kb, 0-3 % n, mixed case."""
    rng = np.random.default_rng([77, seed])
    n = int(rng.integers(50, 401))
    lens = rng.integers(0, 3001, n).astype(np.uint32)
    lens[rng.integers(0, n)] = 0
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20_000)]
    chunks = []
    for L in lens.tolist():
        s = int(rng.integers(0, 20_000 - 3000))
        r = g[s:s + L].copy()
        r[rng.random(L) < rng.random() * 0.03] = ord("n")
        if rng.random() < 0.3:
            r = r | 0x20
        chunks.append(r)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return ReadSet(bases=np.concatenate(chunks), offsets=offs, lengths=lens)


@pytest.mark.parametrize("k,canonical,low,seed", _SWEEP)
def test_gpu_meryl_random_sweep(built, k, canonical, low, seed):
    rs = _ragged(seed)
    want = MN.count_reads(rs, k, canonical, low)
    budget = None if seed % 3 else max(meryl.MIN_BUDGET_BYTES, want.total * 24 // 4)
    mc = _count(rs, k, canonical, low, budget)
    _same(mc, want)
    mc.close()


def test_gpu_meryl_cli_on_reference_store(built, tmp_path):
    """canu's three command lines through bin/meryl on a reference-written gkpStore, then
    bin/estimate-mer-threshold: the files equal the numpy restatement's."""
    import oracle
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "oic_ref")):
        pytest.skip("oracle/_ref/oic_ref not built (no reference sources)")
    from canu_amd import build as B
    rs = synth_reads(120, 3000, 40_000, 0.015, seed=41, n_repeats=3, repeat_len=300)
    P = oracle.default_params(kmer_len=22, max_erate=0.06, min_olap_len=500)
    refwd = str(tmp_path / "ref")
    os.makedirs(refwd)
    oracle.run_reference(rs, P, threads=4, workdir=refwd)
    store = os.path.join(refwd, "w", "ref.gkpStore")
    want = MN.count_reads(rs, 22)
    db = str(tmp_path / "asm.ms22")
    cp = subprocess.run([B.MERYL_CLI_OUT, "-B", "-C", "-L", "2", "-v", "-m", "22", "-threads",
                         "4", "-memory", "1024", "-s", store, "-o", db + ".WORKING"],
                        capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    os.replace(db + ".WORKING.mcdat", db + ".mcdat")
    os.replace(db + ".WORKING.mcidx", db + ".mcidx")
    cp = subprocess.run([B.MERYL_CLI_OUT, "-Dh", "-s", db], capture_output=True, timeout=60)
    assert cp.returncode == 0
    assert cp.stdout == want.histogram_text() and cp.stderr == want.info_text()
    open(db + ".histogram", "wb").write(cp.stdout)
    cp = subprocess.run([B.EMT_CLI_OUT, "-h", db + ".histogram", "-c", "9"],
                        capture_output=True, timeout=60)
    assert cp.returncode == 0
    est = int(cp.stdout)
    assert est == meryl.estimate_threshold(want.histogram_text().decode(), 9)
    thresh = meryl.ovl_threshold(est, 1.0)
    cp = subprocess.run([B.MERYL_CLI_OUT, "-Dt", "-n", str(thresh), "-s", db],
                        capture_output=True, timeout=60)
    assert cp.returncode == 0 and cp.stdout == want.threshold_text(thresh)
    # a FASTA in the store's place counts the same
    fa = str(tmp_path / "reads.fasta")
    with open(fa, "wb") as f:
        for i in range(rs.nreads):
            f.write(b">r%d\n" % i + rs.read(i) + b"\n")
    cp = subprocess.run([B.MERYL_CLI_OUT, "-B", "-C", "-L", "2", "-m", "22", "-s", fa, "-o",
                         db + "f"], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    for ext in (".mcdat", ".mcidx"):
        assert open(db + "f" + ext, "rb").read() == open(db + ext, "rb").read()


def test_gpu_meryl_end_to_end_hand_offs(built, tmp_path):
    """skip_kmers() from the GPU count, fed to OverlapInCore, gives the records of the same
    job fed the golden -Dt fasta through read_skip_fasta; the MHAP hand-off equals the file
    route."""
    from canu_amd.mhap import Mhap, MhapParameters, read_frequency_file
    from canu_amd.overlap_in_core import OicParameters, OverlapInCore, read_skip_fasta
    rs, k, texts, want = MN.golden("b_k22")
    mc = _count(rs, k)
    fa = str(tmp_path / "frequentMers.fasta")
    open(fa, "wb").write(texts["dt"][25])
    P = OicParameters(Kmer_Len=22, maxErate=float(np.float32(0.06)), Min_Olap_Len=100).finalize()
    recs = []
    for skip in (meryl.skip_kmers(mc, 25), read_skip_fasta(fa, 22)):
        oic = OverlapInCore(P, device=0)
        recs.append(oic.run(rs, skip_kmers=skip))
        oic.close()
    assert recs[0].shape[0] > 100 and np.array_equal(recs[0], recs[1])

    m16 = _count(rs, 16)
    gz = str(tmp_path / "ignore.gz")
    ft = 0.00002
    meryl.write_mhap_ignore(m16, ft, gz)
    direct = meryl.mhap_frequencies(m16, ft)
    assert len(direct[0]) > 0
    outs = []
    for fr in (direct, read_frequency_file(gz, 16, with_count=True)):
        mh = Mhap(MhapParameters(k=16).canu_weighting(ft), device=0)
        outs.append(mh.run(rs, frequencies=fr))
        mh.close()
    assert outs[0].shape[0] > 0 and np.array_equal(outs[0], outs[1])
    mc.close()
    m16.close()
