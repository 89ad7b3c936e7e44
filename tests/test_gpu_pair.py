"""libcanu_pair.so and canu_amd/bin/overlapPair on the device: the reference's fixtures record
for record, the aligner's block / stripe / scratch boundaries against the Python restatement
(tests/pair_restate.py, itself pinned to the reference in test_pair_cpu.py), order and
determinism, trivial input, the drop-in executable and the MHAP -> overlapPair chain."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import pair_restate as PR
from canu_amd import pair
from canu_amd.mhap import Mhap, MhapParameters, to_overlaps
from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
from canu_amd.synth import ReadSet, synth_reads

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _params(o: dict) -> pair.PairParameters:
    return pair.PairParameters(o["erate"], o["min_len"], o["partial"], o["invert"])


def _run(rs, recs, P):
    op = pair.OverlapPair(P, device=0)
    try:
        op.load_reads(rs)
        got = op.realign(recs)
        return got, op.counters(), op.stats()
    finally:
        op.close()


def _assert_same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), PR.unpack(got[bad[0]]),
                           PR.unpack(want[bad[0]]))


def _read_set(reads: list[bytes]) -> ReadSet:
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return ReadSet(bases=np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets=offs,
                   lengths=lens, first_iid=1)


# ------------------------------------------------------------------------------ fixtures

@pytest.mark.parametrize("name", PR.FIXTURES)
def test_fixture_equals_reference(built, name):
    rs, inp, want, counters, args = PR.golden(name)
    got, c, st = _run(rs, inp, _params(PR.parse_args(args)))
    _assert_same(got, want, name)
    assert c == counters
    assert st["dp_passes"] > 0 and st["dp_cells"] > 0 and st["ms_kernel"] > 0


# ------------------------------------------------------------------------ aligner shapes

SPANS = (1, 63, 64, 65, 127, 128, 4095, 4096, 4097, 9000)


def _mutated(rng, seq: bytes, err: float) -> bytes:
    out = bytearray()
    for c in seq:
        u = rng.random()
        if u < err / 3:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
        elif u < 2 * err / 3:
            out.append(c)
            out.append(b"ACGT"[int(rng.integers(0, 4))])
        elif u >= err:
            out.append(c)
    return bytes(out) or b"A"


def _shape_cases():
    """Reads and overlaps whose first alignment has a query (B's span) of every length of
    SPANS against a target (all of A: the widening is clipped by the read) that is shorter,
    equal and 1,000 longer; B forward and flipped; N at rows 63/64 and 4095/4096; a pair whose
    columns all tie."""
    rng = np.random.default_rng(20260)
    reads, recs = [], []

    def add(seq):
        reads.append(seq)
        return len(reads)

    for m in SPANS:
        for k, n in enumerate((max(1, m - max(1, m // 8)), m, m + 1000)):
            src = _ACGT[rng.integers(0, 4, max(m, n) + 50)].tobytes()
            q = bytearray(_mutated(rng, src[:m], 0.03))[:m].ljust(m, b"C")
            for p in (63, 64, 4095, 4096):
                if p < m and k == 1:
                    q[p] = ord("N")
            b5, b3 = (m % 7) * 3, (m % 5) * 2                 # B keeps bases outside its span
            bread = _ACGT[rng.integers(0, 4, b5)].tobytes() + bytes(q) + \
                _ACGT[rng.integers(0, 4, b3)].tobytes()
            off = (n - m) // 2 if n > m else 0
            aread = bytearray(src[:n] if n <= m else
                              _ACGT[rng.integers(0, 4, off)].tobytes() + src[:m] +
                              _ACGT[rng.integers(0, 4, n - m - off)].tobytes())
            if k == 1 and m > 64:
                aread[64] = ord("N")
            flipped = (len(recs) % 2) == 1
            a = add(bytes(aread))
            b = add(PR.revcomp(bread) if flipped else bread)
            recs.append(PR.make_record(a, b, 0, 0, b5, b3, flipped))
    # two 9 kb reads sharing 6 kb, reported short of the ends: the dovetail extensions and a
    # global alignment of two stripes
    src = _ACGT[rng.integers(0, 4, 12000)].tobytes()
    for flipped in (False, True):
        bread = _mutated(rng, src[3000:12000], 0.03)
        a = add(_mutated(rng, src[:9000], 0.03))
        b = add(PR.revcomp(bread) if flipped else bread)
        recs.append(PR.make_record(a, b, 3300, 200, 250, 3200, flipped))
    # every column ties: homopolymers, and a period-3 pair
    a, b = add(b"A" * 700), add(b"A" * 300)
    recs.append(PR.make_record(a, b, 100, 200, 10, 20))
    a, b = add(b"ACG" * 300), add(PR.revcomp(b"ACG" * 120))
    recs.append(PR.make_record(a, b, 90, 300, 7, 11, True))
    return _read_set(reads), np.array(recs, dtype=RECORD_DTYPE)


@pytest.fixture(scope="module")
def shapes():
    rs, recs = _shape_cases()
    reads = PR.reads_dict(rs)
    want = {}
    for mode, P in (("partial", pair.PairParameters(0.30, 1, True, False)),
                    ("normal", pair.PairParameters(0.12, 1, False, False))):
        want[mode] = (P, *PR.realign(recs, reads, P.max_erate, 1, P.partial, False))
    return rs, recs, want


@pytest.mark.parametrize("mode", ["partial", "normal"])
def test_aligner_shapes(built, shapes, mode):
    rs, recs, want = shapes
    P, w_rec, w_cnt = want[mode]
    assert w_cnt["nPassed"] > len(SPANS) and w_cnt["nSkipped"] == 0
    if mode == "normal":
        assert w_cnt["nExt5b"] + w_cnt["nExt5a"] >= 2 and w_cnt["nExt3a"] + w_cnt["nExt3b"] >= 2
    got, c, st = _run(rs, recs, P)
    _assert_same(got, w_rec, mode)
    assert c == w_cnt
    assert st["scratch_bytes"] == 0


def test_limit_at_best_and_one_below(built):
    """best == k passes and best == k + 1 fails: erate is chosen against the known distance
    of the first alignment."""
    rng = np.random.default_rng(9)
    src = _ACGT[rng.integers(0, 4, 1500)].tobytes()
    q = bytearray(src[200:1200])
    for p in range(5, 1000, 37):
        q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4]
    rs = _read_set([src, bytes(q)])
    recs = np.array([PR.make_record(1, 2, 150, 250, 0, 0)], dtype=RECORD_DTYPE)
    best = min(PR.bottom_row(bytes(q), src, 0))
    assert best == len(range(5, 1000, 37))
    reads = PR.reads_dict(rs)
    for k, fails in ((best, 0), (best - 1, 1)):
        erate = (k - 0.5) / (1500 * 1.1)
        assert PR.max_edit(1000, 1500, erate) == k
        P = pair.PairParameters(erate, 1, True, False)
        w_rec, w_cnt = PR.realign(recs, reads, erate, 1, True, False)
        assert w_cnt["nFailExtA"] == fails
        got, c, _ = _run(rs, recs, P)
        _assert_same(got, w_rec, k)
        assert c == w_cnt


def test_boundary_row_in_lds_and_in_global_scratch(built):
    """A query of two stripes against a target of exactly PAIR_LDS_COLUMNS columns (the row
    fills LDS) and of one more (the smallest that takes the global scratch row)."""
    rng = np.random.default_rng(31)
    m = pair.STRIPE_ROWS + 1
    P = pair.PairParameters(0.10, 1, True, False)
    rec = np.array([PR.make_record(1, 2, 0, 0, 0, 0)], dtype=RECORD_DTYPE)
    for n in (pair.LDS_COLUMNS, pair.LDS_COLUMNS + 1):
        src = _ACGT[rng.integers(0, 4, n)].tobytes()
        rs = _read_set([src, _mutated(rng, src[6000:6000 + m], 0.02)[:m].ljust(m, b"G")])
        w_rec, w_cnt = PR.realign(rec, PR.reads_dict(rs), P.max_erate, 1, True, False)
        assert w_cnt["nPassed"] == 1 and w_cnt["nFailExtA"] == 0
        got, c, st = _run(rs, rec, P)
        _assert_same(got, w_rec, n)
        assert c == w_cnt
        assert (st["scratch_bytes"] > 0) == (n > pair.LDS_COLUMNS)


# ------------------------------------------------------------------- determinism and order

def test_deterministic_and_order_preserving(built):
    rs, inp, want, counters, args = PR.golden("a")
    P = _params(PR.parse_args(args))
    op = pair.OverlapPair(P, device=0)
    op.load_reads(rs)
    one = op.realign(inp)
    two = op.realign(inp)
    assert one.tobytes() == two.tobytes()
    perm = np.random.default_rng(4).permutation(inp.shape[0])
    shuffled = op.realign(inp[perm])
    assert op.counters() == counters
    back = np.zeros_like(shuffled)
    back[perm] = shuffled
    assert back.tobytes() == one.tobytes()
    _assert_same(one, want, "a")
    assert np.array_equal(one["a"], inp["a"]) and np.array_equal(one["b"], inp["b"])
    # a part of the batch gives that part of the result
    part = op.realign(inp[17:41])
    op.close()
    assert part.tobytes() == one[17:41].tobytes()


def test_empty_and_trivial_input(built):
    rs, inp, want, _, args = PR.golden("d")
    P = _params(PR.parse_args(args))
    op = pair.OverlapPair(P, device=0)
    op.load_reads(rs)
    none = op.realign(inp[:0])
    assert none.shape == (0,) and op.counters() == {k: 0 for k in PR.COUNTERS}
    one = op.realign(inp[5:6])
    _assert_same(one, want[5:6], "one overlap")
    assert op.counters()["nPassed"] + op.counters()["nFailed"] == 1
    # a read against itself, forward: a perfect full-length overlap
    L = int(rs.lengths[2])
    same = np.array([PR.make_record(3, 3, 0, 0, 0, 0), PR.make_record(3, 3, 40, 0, 0, 40)],
                    dtype=RECORD_DTYPE)
    got = op.realign(same)
    w_rec, w_cnt = PR.realign(same, PR.reads_dict(rs), P.max_erate, P.min_overlap_length)
    _assert_same(got, w_rec, "self")
    assert op.counters() == w_cnt
    o = PR.unpack(got[0])
    assert (o["ahg5"], o["ahg3"], o["bhg5"], o["bhg3"], o["evalue"], o["forUTG"]) == \
        (0, 0, 0, 0, 0, 1) and L > 0
    # what the reference would read outside a sequence for is refused
    with pytest.raises(pair.PairError) as e:
        op.realign(np.array([PR.make_record(3, 4, L, 1, 0, 0)], dtype=RECORD_DTYPE))
    assert e.value.code == -4
    with pytest.raises(pair.PairError):
        op.realign(np.array([PR.make_record(3, rs.nreads + 1, 0, 0, 0, 0)], dtype=RECORD_DTYPE))
    op.close()


def test_reads_from_device_buffers_and_bad_bases(built):
    import torch
    rs, inp, want, counters, args = PR.golden("b")
    d_bases = torch.from_numpy(np.array(rs.bases)).cuda()
    d_offs = torch.from_numpy(np.array(rs.offsets).astype(np.int64)).cuda()
    op = pair.OverlapPair(_params(PR.parse_args(args)), device=0)
    op.load_reads_device(rs.first_iid, d_bases.data_ptr(), d_offs.data_ptr(), rs.lengths)
    torch.cuda.synchronize()
    got = op.realign(inp)
    _assert_same(got, want, "b from device buffers")
    assert op.counters() == counters
    bad = ReadSet(bases=np.frombuffer(b"ACGTacgt", dtype=np.uint8).copy(),
                  offsets=np.array([0], dtype=np.uint64), lengths=np.array([8], dtype=np.uint32))
    with pytest.raises(pair.PairError) as e:
        op.load_reads(bad)
    assert e.value.code == -4
    op.close()


# ----------------------------------------------------------------------------- the drop-in

@pytest.mark.skipif(not oracle.reference_available(), reason="oracle/_ref/oic_ref is not built")
@pytest.mark.parametrize("name", PR.FIXTURES)
def test_drop_in_executable(built, tmp_path, name):
    from canu_amd import build as B
    rs, inp, want, counters, args = PR.golden(name)
    gkp = oracle.build_gkpstore(rs, str(tmp_path))
    os.makedirs(str(tmp_path / "results"))
    src = str(tmp_path / "results" / "000001.mhap.ovb")
    dst = str(tmp_path / "results" / "000001.WORKING.ovb")
    write_ovb(inp, src, counts=False)
    cp = subprocess.run([B.PAIR_CLI_OUT, "-G", gkp, "-O", src, "-o", dst, *args, "-memory", "4",
                         "-t", "2"], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    _assert_same(oracle.read_ovb_reference(dst), want, name)
    assert PR.parse_report(cp.stderr) == counters
    tot = counters["nPassed"] + counters["nFailed"]
    assert f" -- {counters['nFailed']} failed {counters['nPassed']} passed " \
           f"({100.0 * counters['nPassed'] / tot:.4f}%).\n" in cp.stderr
    # the reference leaves <base>.counts beside its output (ovFileFullWrite)
    cnt = np.fromfile(str(tmp_path / "results" / "000001.counts"), dtype="<u4")
    opr = np.bincount(np.concatenate([want["a"], want["b"]]), minlength=int(cnt[0]))
    assert np.array_equal(cnt[1:], opr)


def test_drop_in_refusals(built, tmp_path):
    from canu_amd import build as B
    for argv, word in ((["-G", "g", "-O", str(tmp_path), "-o", "o", "-len", "500"], "directory"),
                       (["-G", "g", "-O", "i", "-o", "o"], "-len 0"),
                       (["-G", "g", "-O", "i"], "usage"),
                       (["-G", "g", "-O", "i", "-o", "o", "-frobnicate"], "usage")):
        cp = subprocess.run([B.PAIR_CLI_OUT, *argv], capture_output=True, text=True, timeout=60)
        assert cp.returncode == 1 and word in cp.stderr, (argv, cp.stderr)


# ------------------------------------------------------------------------------- the chain

def test_mhap_to_overlap_pair_chain(built):
    """Mhap.run -> to_overlaps -> OverlapPair.realign with no reference tool in between; the
    result is the restatement's on the same input."""
    rs = synth_reads(n_reads=40, read_len=3000, genome_len=10_000, error_rate=0.03, seed=3)
    m = Mhap(MhapParameters(), device=0)
    hits = m.run(rs)
    m.close()
    ovl = to_overlaps(hits, rs)
    assert ovl.shape[0] > 50
    ovl = ovl[:120]
    P = pair.PairParameters(0.12, 500, False, False)
    got, c, _ = _run(rs, ovl, P)
    w_rec, w_cnt = PR.realign(ovl, PR.reads_dict(rs), P.max_erate, P.min_overlap_length)
    _assert_same(got, w_rec, "chain")
    assert c == w_cnt and c["nPassed"] > 20
    passed = got[(got["w0"] >> np.uint64(42)) & np.uint64(0xfff) != 4095]
    assert passed.shape[0] == c["nPassed"]
