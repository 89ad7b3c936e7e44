"""trimReads on the GPU (libcanu_tr.so, canu_amd/bin/trimReads) against the reference's own
files (tests/golden/tr_*.npz) and, on inputs the reference was not run on, against its
restatement (tests/tr_restate.py, pinned to the same files by test_tr_cpu.py)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tr_restate as TR  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("a", "b0", "b1", "b2", "b3", "c", "d")
REC = np.dtype([("a", "<u4"), ("b", "<u4"), ("w0", "<u8"), ("w1", "<u8")])


def fixture(name):
    fx = np.load(os.path.join(GOLDEN, f"tr_{name}.npz"))
    args = fx["args"].tobytes().decode().split()
    return fx, args


def params_of(args):
    from canu_amd.trim_reads import parse_trimReads_args
    P, job = parse_trimReads_args(args + ["-G", "g", "-O", "o", "-Co", "c", "-o", "p"])
    rng = (job["id_min"], job["id_max"]) if "-t" in args else None
    return P, rng


@pytest.fixture(scope="module")
def tr():
    from canu_amd.trim_reads import TrimReads
    t = TrimReads()
    yield t
    t.close()


def restated(lengths, records, rules, P, id_range=None):
    rp = TR.Params(P.erate, P.min_read_length, P.min_evidence_overlap, P.min_evidence_coverage)
    return TR.trim_reads(lengths, records, rules, rp, id_range), rp


def check(tr, lengths, records, rules=1, P=None, id_range=None):
    """The library's arrays, counters and texts equal the restatement's."""
    from canu_amd.trim_reads import FLAG_NO_HQ, FLAG_RESET, TrParameters
    P = P or TrParameters()
    tr.set_params(P)
    records = np.asarray(records, dtype=REC)
    got = tr.run(lengths, records, rules, id_range)
    want, rp = restated(lengths, records, rules, P, id_range)
    for k in ("status", "bgn", "end", "n_skipped", "n_used"):
        bad = np.flatnonzero(getattr(got, k) != want[k])
        assert bad.size == 0, (k, bad[:5] + 1, getattr(got, k)[bad[:5]], want[k][bad[:5]])
    assert np.array_equal((got.flags & FLAG_NO_HQ) != 0, want["no_hq"] != 0)
    assert np.array_equal((got.flags & FLAG_RESET) != 0, want["reset"] != 0)
    assert got.counters == want["counters"]
    assert got.clear_bytes() == TR.clear_bytes(want)
    assert got.log_text() == TR.log_text(want)
    assert got.stats_text() == TR.stats_text(want, rp)
    assert got.stderr_text() == TR.stderr_text(want)
    return got


def records_of(per_read, lengths, rng=None):
    """per_read: for read k + 1 a list of (bgn, end[, evalue]) -> sorted records."""
    out = []
    for k, ivs in enumerate(per_read):
        for j, iv in enumerate(ivs):
            b = int(rng.integers(1, len(per_read) + 1)) if rng is not None else 1 + (j % len(per_read))
            out.append(TR.make_record(k + 1, b, iv[0], iv[1], int(lengths[k]), iv[2] if len(iv) > 2 else 0, 4))
    return np.array(out, dtype=REC) if out else np.zeros(0, dtype=REC)


def random_intervals(rng, n, length, grid=1, bad=0.1):
    lo = rng.integers(0, length // grid, n) * grid
    hi = np.minimum(lo + rng.integers(1, max(2, length // grid // 2), n) * grid, length)
    lo = np.minimum(lo, hi - 1)
    ev = np.where(rng.random(n) < bad, TR.BAD_EV, 0)
    return [(int(a), int(b), int(e)) for a, b, e in zip(lo, hi, ev)]


# ------------------------------------------------------------------ the reference's files

@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_library(tr, name):
    fx, args = fixture(name)
    P, rng = params_of(args)
    tr.set_params(P)
    got = tr.run(fx["lengths"], fx["records"], fx["rules"], rng)
    assert got.clear_bytes() == fx["clear"].tobytes()
    assert got.log_text().encode() == fx["log"].tobytes()
    assert got.stats_text().encode() == fx["stats"].tobytes()
    assert got.stderr_text().encode() == fx["stderr"].tobytes()


def test_fixture_executable(tmp_path):
    """canu_amd/bin/trimReads on the stores the reference wrote, with canu's command line."""
    fx, args = fixture("d")
    for tag in ("gkp", "ovs"):
        d = tmp_path / tag
        d.mkdir()
        for f in fx[tag + "_names"]:
            (d / str(f)).write_bytes(fx[f"{tag}_file_{f}"].tobytes())
    exe = os.path.join(ROOT, "canu_amd", "bin", "trimReads")
    pre = str(tmp_path / "asm.1.trimReads")
    cmd = [exe, "-G", str(tmp_path / "gkp"), "-O", str(tmp_path / "ovs"), "-Co", pre + ".clear", *args, "-o", pre]
    cp = subprocess.run(cmd, capture_output=True)
    assert cp.returncode == 0, cp.stderr
    assert cp.stderr == fx["stderr"].tobytes()
    for ext in ("clear", "log", "stats"):
        assert open(f"{pre}.{ext}", "rb").read() == fx[ext].tobytes(), ext
    assert sorted(os.listdir(tmp_path)) == ["asm.1.trimReads.clear", "asm.1.trimReads.log",
                                            "asm.1.trimReads.stats", "gkp", "ovs"]   # no plots
    # a second run loads the clear file the first wrote, resets it and writes the same
    cp = subprocess.run(cmd, capture_output=True)
    assert cp.returncode == 0 and open(pre + ".clear", "rb").read() == fx["clear"].tobytes()
    for opt in ("-Ci", "-Cm", "-l"):
        cp = subprocess.run(cmd + [opt, "x"], capture_output=True)
        assert cp.returncode == 1 and b"not supported" in cp.stderr.splitlines()[0]
    cp = subprocess.run([a for a in cmd if a not in ("-Co", pre + ".clear")], capture_output=True)
    assert cp.returncode == 1 and b"-Co" in cp.stderr.splitlines()[0]


# ------------------------------------------------------------------ sizes

def test_zero_one_two_overlaps(tr):
    lengths = [1000, 1000, 1000, 1000]
    check(tr, lengths, records_of([[], [(100, 900)], [(0, 500), (450, 1000)], []], lengths))
    check(tr, lengths, np.zeros(0, dtype=REC))


@pytest.mark.parametrize("oc", [1, 2])
def test_overlap_counts_around_the_wave_and_the_capacity(tr, oc):
    from canu_amd.trim_reads import TrParameters, wave_capacity
    cap = wave_capacity()
    rng = np.random.default_rng(40 + oc)
    counts = [31, 32, 33, 63, 64, 65, cap - 1, cap, cap + 1]
    lengths = [5000] * len(counts)
    per = [random_intervals(rng, c, 5000, grid=10) for c in counts]
    got = check(tr, lengths, records_of(per, lengths, rng), rules=[1, 2] * 4 + [1],
                P=TrParameters(min_evidence_coverage=oc))
    assert got.stats["n_large_reads"] == 1 and got.stats["n_wave_reads"] == len(counts) - 1
    check(tr, lengths, records_of(per, lengths, rng), rules=2, P=TrParameters(min_evidence_coverage=oc))


def test_twenty_thousand_overlaps(tr):
    """One read with 20,000 identical overlaps, one with 20,000 distinct pairs of end points."""
    from canu_amd.trim_reads import TrParameters
    n = 20_000
    lengths = [3000, 100_000]
    per = [[(100, 2900)] * n, [(2 * k, 50_001 + 2 * k) for k in range(n)]]
    for oc in (1, 3):
        got = check(tr, lengths, records_of(per, lengths), P=TrParameters(min_evidence_coverage=oc))
        assert got.stats["n_large_reads"] == 2
        assert (int(got.bgn[0]), int(got.end[0])) == (100, 2900)


# ------------------------------------------------------------------ the hand-made cases, moved

def test_hand_made_cases_at_random_positions(tr):
    from canu_amd.trim_reads import TrParameters
    rng = np.random.default_rng(77)
    for oc in (0, 1, 2, 3):
        for rule, cases in ((1, TR.CASES_B), (2, TR.CASES_C)):
            per, lengths = [], []
            for name, ivs in cases * 3:
                s = int(rng.integers(0, 700))
                if name == "wrap":                      # the first interval ends below -ol
                    per.append([(0, int(rng.integers(1, 40))), (500 + s, 900 + s)])
                else:
                    per.append([(iv[0] + s, iv[1] + s) + tuple(iv[2:]) for iv in ivs])
                lengths.append(1000 + s + int(rng.integers(0, 2)) * int(rng.integers(0, 300)))
            check(tr, lengths, records_of(per, lengths, rng), rules=rule,
                  P=TrParameters(min_evidence_coverage=oc))


def test_coverage_and_overlap_options(tr):
    from canu_amd.trim_reads import TrParameters
    rng = np.random.default_rng(5)
    lengths = [int(v) for v in rng.integers(300, 1200, 60)]
    per = [random_intervals(rng, int(rng.integers(0, 14)), L, grid=int(rng.choice([1, 10, 50]))) for L in lengths]
    rec = records_of(per, lengths, rng)
    rules = rng.integers(1, 3, 60)
    literal = 0
    for oc in (0, 1, 2, 3):
        for ol in (0, 1, 40):
            got = check(tr, lengths, rec, rules, TrParameters(min_evidence_overlap=ol, min_evidence_coverage=oc))
            assert oc >= 2 or got.stats["n_literal"] == 0
            literal += got.stats["n_literal"]
    assert literal > 0                                  # some reads took the event-by-event walk


@pytest.mark.parametrize("points", [1, 64, 65])
def test_best_edge_trim_points(tr, points):
    lengths = [6000, 6000, 6000]
    fwd = [(10 * j, 5000 + j) for j in range(points)]
    per = [fwd, [(6000 - e, 6000 - b) for b, e in fwd], fwd + [(6000 - e, 6000 - b) for b, e in fwd]]
    check(tr, lengths, records_of(per, lengths), rules=2)


def test_minlength_and_erate(tr):
    from canu_amd.trim_reads import TrParameters
    lengths = [1000] * 4
    per = [[(100, 163)], [(100, 164)], [(0, 900, 150), (50, 1000, 151)], [(0, 1000, 4095)]]
    check(tr, lengths, records_of(per, lengths))
    check(tr, lengths, records_of(per, lengths), P=TrParameters(erate=0.5, min_read_length=0))


# ------------------------------------------------------------------ order, repeats, ranges, errors

def test_order_within_a_read_and_two_runs(tr):
    rng = np.random.default_rng(9)
    lengths = [2000] * 30
    per = [random_intervals(rng, int(rng.integers(1, 40)), 2000, grid=20) for _ in lengths]
    rec = records_of(per, lengths, rng)
    one = check(tr, lengths, rec, rules=2)
    two = tr.run(lengths, rec, 2)
    key = rng.random(rec.shape[0])
    shuffled = rec[np.lexsort((key, rec["a"]))]
    three = tr.run(lengths, shuffled, 2)
    for other in (two, three):
        for k in ("bgn", "end", "status", "flags", "n_skipped", "n_used"):
            assert np.array_equal(getattr(one, k), getattr(other, k)), k
        assert one.counters == other.counters


def test_id_range(tr):
    rng = np.random.default_rng(10)
    lengths = [1500] * 20
    per = [random_intervals(rng, 6, 1500) for _ in lengths]
    rec = records_of(per, lengths, rng)
    for r in ((5, 12), (1, 1), (20, 500), (0, 3), (15, 14)):
        got = check(tr, lengths, rec, id_range=r)
        lo, hi = max(r[0], 1), min(r[1], 20)
        outside = np.ones(20, bool)
        outside[lo - 1:hi] = False
        assert (got.status[outside] == 0).all() and (got.status[~outside] != 0).all()
        b, e = got.clear_ranges()
        assert (b[outside] == 0).all() and (e[outside] == 1500).all()


def test_error_returns(tr):
    from canu_amd.trim_reads import TrError
    lengths = [1000, 1000, 1000]
    good = records_of([[(0, 500)], [(100, 900)], [(5, 700)]], lengths)
    cases = {
        "not sorted": good[[1, 0, 2]],
        "outside": np.array([TR.make_record(4, 1, 0, 500, 1000, 0, 4)], dtype=REC),
        "read 0": np.array([TR.make_record(0, 1, 0, 500, 1000, 0, 4)], dtype=REC),
        "a_bgn >= a_end": np.array([(1, 2, 600 | (400 << 21), 0)], dtype=REC),
    }
    for what, rec in cases.items():
        with pytest.raises(TrError) as e:
            tr.run(lengths, rec)
        assert e.value.code == -4, what
    with pytest.raises(TrError) as e:                   # a read of the range without a rule
        tr.run(lengths, good, rules=[1, 0, 1])
    assert e.value.code == -4
    tr.run(lengths, good, rules=[1, 0, 1], id_range=(3, 3))   # outside the range it does not matter
    with pytest.raises(TrError):
        tr.run([1 << 21], np.zeros(0, dtype=REC))
    check(tr, lengths, good)                            # and the context still works


# ------------------------------------------------------------------ the chain

def test_chain_from_the_overlapper(tr):
    """OverlapInCore.run -> store_view -> TrimReads.run, no file in between."""
    from canu_amd.find_errors import store_view
    from canu_amd.overlap_in_core import OicParameters, OverlapInCore
    from canu_amd.synth import synth_reads
    from canu_amd.trim_reads import TrParameters
    rs = synth_reads(n_reads=60, read_len=1500, genome_len=12_000, error_rate=0.01, seed=21)
    P = OicParameters(Kmer_Len=22, maxErate=float(np.float32(0.06)), Min_Olap_Len=100,
                      Doing_Partial_Overlaps=True).finalize()
    oic = OverlapInCore(P, device=0)
    view = store_view(oic.run(rs))
    oic.close()
    assert view.shape[0] > 100
    got = check(tr, rs.lengths, view, P=TrParameters(erate=0.03, min_read_length=500, min_evidence_coverage=2))
    assert got.stats["n_overlaps"] == view.shape[0]
