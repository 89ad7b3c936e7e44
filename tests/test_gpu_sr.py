"""splitReads on the GPU (libcanu_sr.so, canu_amd/bin/splitReads) against the reference's own
files (tests/golden/sr_*.npz) and, on inputs the reference was not run on, against its
restatement (tests/sr_restate.py, pinned to the same files by test_sr_cpu.py)."""
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

import sr_restate as SR  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("a", "b", "c", "d")
REC = np.dtype([("a", "<u4"), ("b", "<u4"), ("w0", "<u8"), ("w1", "<u8")])
U32 = 0xFFFFFFFF
LEN = 8000


def fixture(name):
    fx = np.load(os.path.join(GOLDEN, f"sr_{name}.npz"))
    from canu_amd.split_reads import parse_splitReads_args
    P, job = parse_splitReads_args(fx["args"].tobytes().decode().split() + "-G g -O o -Co c -o p".split())
    return fx, P, (job["id_min"], job["id_max"])


@pytest.fixture(scope="module")
def sr():
    from canu_amd.split_reads import SplitReads
    s = SplitReads()
    yield s
    s.close()


def compare(got, want, rp, records):
    for k in ("status", "bgn", "end", "n_adjusted", "n_bad_regions", "fate"):
        bad = np.flatnonzero(getattr(got, k) != want[k])
        assert bad.size == 0, (k, bad[:5] + 1, getattr(got, k)[bad[:5]], want[k][bad[:5]])
    assert [tuple(int(v) for v in r) for r in got.regions] == want["regions"]
    assert np.array_equal(got.region_off, want["region_off"])
    assert got.counters == want["counters"]
    assert (got.id_min, got.id_max) == (want["id_min"], want["id_max"])
    assert got.clear_bytes() == SR.clear_bytes(want)
    assert got.log_text() == SR.log_text(want)
    assert got.stats_text() == SR.stats_text(want, rp)
    assert got.stderr_text() == SR.stderr_text(want, rp, records)


def check(sr, lengths, records, lib_flags=3, clear=None, P=None, id_range=None):
    """The library's arrays, fate, regions, counters and texts equal the restatement's; where the
    restatement refuses the input, so does the library."""
    from canu_amd.split_reads import SrError, SrParameters
    P = P or SrParameters()
    sr.set_params(P)
    records = np.asarray(records, dtype=REC)
    rp = SR.Params(P.erate, P.min_read_length)
    try:
        want = SR.split_reads(lengths, records, lib_flags, clear, rp, id_range)
    except SR.BadInput:
        with pytest.raises(SrError) as e:
            sr.run(lengths, records, lib_flags, clear, id_range)
        assert e.value.code == -4
        return None
    got = sr.run(lengths, records, lib_flags, clear, id_range)
    compare(got, want, rp, records)
    return got


def sort_records(recs):
    """By (a_iid, b_iid), the given order kept within a pair."""
    r = np.array(recs, dtype=REC) if len(recs) else np.zeros(0, dtype=REC)
    key = (r["a"].astype(np.uint64) << np.uint64(32)) | r["b"].astype(np.uint64)
    return r[np.argsort(key, kind="stable")]


class Job:
    """Reads of LEN bases; every overlap pair of a read takes the next partner, so that the
    order of a read's records is the order they were added in."""

    def __init__(self, n_reads, length=LEN):
        self.lengths = [length] * n_reads
        self.recs = []
        self.next_b = {}

    def partner(self, a):
        b = self.next_b.get(a, 0) + 1
        if b == a:
            b += 1
        self.next_b[a] = b
        assert b <= len(self.lengths), "more partners than reads"
        return b

    def single(self, a, abgn, aend, bbgn=1000, bend=1400, flipped=False, b=None):
        b = b or self.partner(a)
        self.recs.append(SR.make_record(a, b, abgn, aend, self.lengths[a - 1], bbgn, bend,
                                        self.lengths[b - 1], flipped))

    def twins(self, a, lo, hi, arm=100):
        """A forward overlap ending at lo and a flipped one starting at hi, on one stretch of B."""
        b = self.partner(a)
        self.single(a, lo - arm, lo, b=b)
        self.single(a, hi, hi + arm, flipped=True, b=b)

    def records(self):
        return sort_records(self.recs)


# ------------------------------------------------------------------ the reference's files

@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_library(sr, name):
    fx, P, rng = fixture(name)
    sr.set_params(P)
    clear = tuple(fx["clear_in"])
    got = sr.run(fx["lengths"], fx["records"], fx["lib_flags"], clear, rng)
    e0 = (0, 0)
    if "clear_in_file" in fx:
        b, e = SR.parse_clear(fx["clear_in_file"].tobytes())
        e0 = (int(b[0]), int(e[0]))
    assert got.clear_bytes(entry0=e0) == fx["clear"].tobytes()
    assert got.log_text().encode() == fx["log"].tobytes()
    assert got.stats_text().encode() == fx["stats"].tobytes()
    assert got.stderr_text().encode() == fx["stderr"].tobytes()
    rp = SR.Params(P.erate, P.min_read_length)
    compare(got, SR.split_reads(fx["lengths"], fx["records"], fx["lib_flags"], clear, rp, rng), rp, fx["records"])


def test_fixture_executable(tmp_path):
    """canu_amd/bin/splitReads on the stores the reference wrote, with canu's command line."""
    fx, P, rng = fixture("d")
    args = fx["args"].tobytes().decode().split()
    for tag in ("gkp", "ovs"):
        d = tmp_path / tag
        d.mkdir()
        for f in fx[tag + "_names"]:
            (d / str(f)).write_bytes(fx[f"{tag}_file_{f}"].tobytes())
    ci = str(tmp_path / "asm.1.trimReads.clear")
    open(ci, "wb").write(fx["clear_in_file"].tobytes())
    exe = os.path.join(ROOT, "canu_amd", "bin", "splitReads")
    pre = str(tmp_path / "asm.2.splitReads")
    base = [exe, "-G", str(tmp_path / "gkp"), "-O", str(tmp_path / "ovs")]
    cmd = base + ["-Ci", ci, "-Co", pre + ".clear", *args, "-o", pre]
    cp = subprocess.run(cmd, capture_output=True)
    assert cp.returncode == 0, cp.stderr
    assert cp.stderr == fx["stderr"].tobytes()
    for ext in ("clear", "log", "stats"):
        assert open(f"{pre}.{ext}", "rb").read() == fx[ext].tobytes(), ext
    # a second run loads the clear file the first wrote, resets it and writes the same
    cp = subprocess.run(cmd, capture_output=True)
    assert cp.returncode == 0 and open(pre + ".clear", "rb").read() == fx["clear"].tobytes()
    # its own output as the input: the restatement on those clear ranges
    rp = SR.Params(P.erate, P.min_read_length)
    n = int(fx["lengths"].shape[0])
    pre3 = str(tmp_path / "again")
    cp = subprocess.run(base + ["-Ci", pre + ".clear", "-Co", pre3 + ".clear", *args, "-o", pre3], capture_output=True)
    assert cp.returncode == 0, cp.stderr
    b, e = SR.parse_clear(fx["clear"].tobytes(), n)
    want = SR.split_reads(fx["lengths"], fx["records"], fx["lib_flags"], (b[1:], e[1:]), rp, rng)
    assert open(pre3 + ".clear", "rb").read() == SR.clear_bytes(want, (int(b[0]), int(e[0])))
    assert open(pre3 + ".stats").read() == SR.stats_text(want, rp)
    assert cp.stderr.decode() == SR.stderr_text(want, rp, fx["records"])
    # no -Ci: every read starts at 0 .. length
    pre4 = str(tmp_path / "fresh")
    cp = subprocess.run(base + ["-Co", pre4 + ".clear", *args, "-o", pre4], capture_output=True)
    assert cp.returncode == 0, cp.stderr
    want = SR.split_reads(fx["lengths"], fx["records"], fx["lib_flags"], None, rp, rng)
    assert open(pre4 + ".clear", "rb").read() == SR.clear_bytes(want)
    assert open(pre4 + ".stats").read() == SR.stats_text(want, rp)
    assert open(pre4 + ".log", "rb").read() == b""
    # the refusals
    cp = subprocess.run(cmd + ["-x", "1"], capture_output=True)
    assert cp.returncode == 1 and cp.stderr.count(b"\n") == 1 and b"unknown option '-x'" in cp.stderr
    cp = subprocess.run([a for a in cmd if a not in ("-Co", pre + ".clear")], capture_output=True)
    assert cp.returncode == 1 and b"-Co" in cp.stderr.splitlines()[0]
    cp = subprocess.run([a for a in cmd if a not in ("-o", pre)], capture_output=True)
    assert cp.returncode == 1 and b"usage" in cp.stderr
    raw = fx["clear_in_file"].tobytes()
    for damaged in (raw[:-4], raw[:3], (n + 1).to_bytes(4, "little") + raw[4:]):
        open(ci, "wb").write(damaged)
        cp = subprocess.run(cmd, capture_output=True)
        assert cp.returncode == 1 and b"clear range file" in cp.stderr


# ------------------------------------------------------------------ sizes

def test_zero_one_two_records(sr):
    J = Job(5)
    J.single(2, 100, 900)
    J.twins(3, 3000, 3010)
    check(sr, J.lengths, J.records())
    check(sr, J.lengths, np.zeros(0, dtype=REC))
    check(sr, [], np.zeros(0, dtype=REC))


def test_record_counts_around_the_wave_and_the_capacity(sr):
    from canu_amd.split_reads import wave_capacity
    cap = wave_capacity()
    counts = [63, 64, 65, cap - 1, cap, cap + 1]
    J = Job(cap + 8)
    a = 0
    for c in counts:
        for lead in (0, 1):     # lead 1: a pair lies on records 63 and 64; lead 0: the last ends at c
            a += 1
            left = c
            if lead:
                J.single(a, 0, 500)
                left -= 1
            for k in range(left // 2):
                lo = 3000 + 40 * (k % 7)
                J.twins(a, lo, lo + (k * 7) % 31)
            if left % 2:
                J.single(a, 7000, 7500)
    rec = J.records()
    assert np.array_equal(np.bincount(rec["a"])[1:a + 1], np.repeat(counts, 2))
    got = check(sr, J.lengths, rec)
    assert got.stats["n_large_reads"] == 2 and got.stats["n_wave_reads"] == 2 * len(counts) - 2
    assert (got.status[:a] == SR.TRIMMED).all()


@pytest.mark.parametrize("layout", ["disjoint", "touching", "nested"])
@pytest.mark.parametrize("count", [1, 64, 65])
def test_bad_interval_counts(sr, layout, count):
    """count bad intervals in one read, each from three twin pairs (and, in a second read, from
    two: too weak unless they fuse)."""
    J = Job(3 * count + 4, 12000)
    for a, copies in ((1, 3), (2, 2)):
        for k in range(count):
            lo, hi = {"disjoint": (1000 + 100 * k, 1010 + 100 * k), "touching": (1000 + 10 * k, 1010 + 10 * k),
                      "nested": (5000 - k, 5000 + k)}[layout]
            for _ in range(copies):
                J.twins(a, lo, hi)
    got = check(sr, J.lengths, J.records())
    assert got.n_bad_regions[0] == (count if layout == "disjoint" else 1)
    assert got.n_bad_regions[1] == (0 if layout == "disjoint" or count == 1 else 1)


def test_twenty_thousand_records(sr):
    """One read with 20,000 records: 5,000 twin pairs planting one junction and 10,000 others."""
    n = 20_000
    J = Job(15_002, 6000)
    for k in range(n // 4):
        J.twins(1, 3000, 3010)
    for k in range(n // 2):
        J.single(1, 10 + k % 50, 1000 + k % 50)
    got = check(sr, J.lengths, J.records())
    assert got.stats["n_large_reads"] == 1 and got.n_adjusted[0] == n
    assert [tuple(r) for r in got.regions.tolist()] == [(1, 3000, 3010)]
    assert (int(got.bgn[0]), int(got.end[0])) == (0, 3000)


# ------------------------------------------------------------------ random jobs

def random_job(seed, n_reads=60):
    rng = np.random.default_rng(seed)
    grid = int(rng.choice([1, 10, 50]))
    lens = (rng.integers(40, 120, n_reads) * 50).astype(np.int64)
    cb, ce = np.zeros(n_reads, np.int64), lens.copy()
    for i in np.flatnonzero(rng.random(n_reads) < 0.2):
        cb[i] = int(rng.integers(0, lens[i] // 4 // grid + 1)) * grid
        ce[i] = lens[i] - int(rng.integers(0, lens[i] // 4 // grid + 1)) * grid
    gone = rng.random(n_reads) < 0.05
    cb[gone] = ce[gone] = U32
    libs = rng.choice([0, 1, 3, 3, 3], n_reads)
    recs = []

    def span(length, lo_min=0):
        lo = int(rng.integers(lo_min // grid, (length - 300) // grid)) * grid
        return lo, min(length, lo + int(rng.integers(1, 40)) * max(grid, 10))

    for a in range(1, n_reads + 1):
        la = int(lens[a - 1])
        m = int(rng.integers(0, min(41, n_reads - 4)))
        partners = rng.permutation(np.delete(np.arange(1, n_reads + 1), a - 1))
        junction = int(rng.integers(600 // grid, (la - 600) // grid)) * grid
        k = 0
        while m > 0:
            b = int(partners[k])
            k += 1
            lb = int(lens[b - 1])
            kind = rng.random()
            if kind < 0.5 and m >= 2:                    # twins around the read's junction
                gap = int(rng.integers(0, 60)) * grid if rng.random() < 0.8 else int(rng.integers(0, 2500))
                arm = int(rng.integers(2, 12)) * 50
                lo, hi = junction + int(rng.integers(-2, 3)) * grid, junction + gap
                f = (max(0, lo - arm), lo)
                g = (min(hi, la - 1), min(la, hi + arm))
                bs = span(lb)
                b2 = bs if rng.random() < 0.7 else span(lb)
                flips = (False, True) if rng.random() < 0.9 else (False, False)
                if rng.random() < 0.5:
                    f, g = g, f
                recs.append(SR.make_record(a, b, f[0], f[1], la, bs[0], bs[1], lb, flips[0]))
                recs.append(SR.make_record(a, b, g[0], g[1], la, b2[0], b2[1], lb, flips[1]))
                m -= 2
                if rng.random() < 0.05 and m >= 1:       # a group of three
                    s = span(la)
                    recs.append(SR.make_record(a, b, s[0], s[1], la, bs[0], bs[1], lb, True))
                    m -= 1
            else:
                s, t = span(la), span(lb)
                recs.append(SR.make_record(a, b, s[0], s[1], la, t[0], t[1], lb, rng.random() < 0.5))
                m -= 1
    return lens, sort_records(recs), libs.astype(np.uint8), (cb, ce)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_random_jobs(sr, seed):
    from canu_amd.split_reads import SrParameters
    lens, rec, libs, clear = random_job(seed)
    done = 0
    for ml in (0, 64, 1000):
        done += check(sr, lens, rec, libs, clear, SrParameters(min_read_length=ml)) is not None
    check(sr, lens, rec, 3, None, SrParameters(erate=0.3))
    assert done == 3


def test_random_jobs_find_regions(sr):
    lens, rec, libs, clear = random_job(2)
    got = check(sr, lens, rec, 3, None)
    assert got.regions.shape[0] > 5 and (got.status == SR.TRIMMED).sum() > 5


def test_exact_half_adjusts(sr):
    """A cut of one base in 2m on A is half a base of m on B (q halves of q * m): round() takes it
    away from zero, and the B sides of a pair then share 249 bases, one too few.  With the halves
    rounded down every read would have a bad region."""
    lens, clear_b, clear_e = [6000] * 8, [0] * 8, [6000] * 8     # the partners
    recs = []
    for m in range(252, 402):
        for q in (1, 3):
            a = len(lens) + 1
            lens.append(6000)
            clear_b.append(1001)
            clear_e.append(6000)
            up = (q + 1) // 2
            for b in (1, 2, 3):
                recs.append(SR.make_record(a, b, 1000, 1000 + 2 * m, 6000, 0, q * m, 6000))
                recs.append(SR.make_record(a, b, 1010 + 2 * m, 1410 + 2 * m, 6000, 0, 249 + up, 6000, True))
    rec = sort_records(recs)
    br = {}
    want = SR.split_reads(lens, rec, 3, (clear_b, clear_e), SR.Params(), branches=br)
    assert br.get("adjust_half", 0) >= 100, br
    halves = br["adjust_half"] // 3
    got = check(sr, lens, rec, 3, (clear_b, clear_e))
    # a read whose product is exactly x.5 has no region; where the double falls just below the
    # half (and rounds down) it has one
    assert int((got.n_bad_regions[8:] == 0).sum()) >= halves
    assert np.array_equal(got.n_bad_regions, want["n_bad_regions"])


# ------------------------------------------------------------------ order, repeats, ranges, errors

def test_order_within_a_pair_and_two_runs(sr):
    lens, rec, libs, clear = random_job(11)
    one = check(sr, lens, rec, 3, None)
    two = sr.run(lens, rec, 3)
    for k in ("bgn", "end", "status", "fate", "n_adjusted", "n_bad_regions"):
        assert np.array_equal(getattr(one, k), getattr(two, k)), k
    assert one.counters == two.counters and np.array_equal(one.regions, two.regions)
    # the two records of every pair swapped: the restatement on that order
    swapped = rec.copy()
    i = 0
    while i + 1 < rec.shape[0]:
        if rec["a"][i] == rec["a"][i + 1] and rec["b"][i] == rec["b"][i + 1]:
            swapped[i], swapped[i + 1] = rec[i + 1], rec[i]
            i += 2
        else:
            i += 1
    check(sr, lens, swapped, 3, None)


def test_id_range(sr):
    lens, rec, libs, clear = random_job(12, 30)
    for r in ((5, 12), (1, 1), (20, 500), (0, 3), (15, 14), (31, 40)):
        got = check(sr, lens, rec, 3, clear, id_range=r)
        lo, hi = max(r[0], 1), min(r[1], 30)
        outside = np.ones(30, bool)
        outside[lo - 1:hi] = False
        assert (got.status[outside] == 0).all() and (got.status[~outside] != 0).all()
        b, e = got.clear_ranges()
        assert np.array_equal(b[outside], clear[0][outside]) and np.array_equal(e[outside], clear[1][outside])
        assert (got.fate[np.isin(rec["a"], np.flatnonzero(outside) + 1)] == 0).all()


def test_error_returns(sr):
    from canu_amd.split_reads import SrError
    lengths = [2000, 2000, 2000]
    good = sort_records([SR.make_record(1, 2, 0, 500, 2000, 0, 500, 2000),
                         SR.make_record(2, 1, 100, 900, 2000, 100, 900, 2000),
                         SR.make_record(2, 3, 100, 900, 2000, 100, 900, 2000),
                         SR.make_record(3, 1, 5, 700, 2000, 5, 700, 2000)])
    one = lambda *r: np.array([r], dtype=REC)  # noqa: E731
    cases = {
        "not sorted by a": (good[[1, 0, 2, 3]], None),
        "not sorted by b": (good[[0, 2, 1, 3]], None),
        "a outside": (one(4, 1, 0, 0), None),
        "b outside": (one(1, 4, 0, 0), None),
        "read 0": (one(0, 1, 0, 0), None),
        "b read 0": (one(1, 0, 0, 0), None),
        "a_bgn >= a_end": (one(1, 2, 1200 | (800 << 21), 0), None),
        "b_bgn >= b_end": (one(1, 2, 0, 1200 | (800 << 21)), None),
        "a hang longer than the read": (one(1, 2, 2500, 0), None),
        "b hang longer than the read": (one(1, 2, 0, 2500 << 21), None),
        "clear bgn > end": (good, ([0, 900, 0], [2000, 800, 2000])),
        "clear end > length": (good, ([0, 0, 0], [2000, 2001, 2000])),
        "half a deleted mark": (good, ([0, U32, 0], [2000, 2000, 2000])),
    }
    for what, (rec, clear) in cases.items():
        with pytest.raises(SR.BadInput):
            SR.split_reads(lengths, rec, 3, clear, SR.Params())
        with pytest.raises(SrError) as e:
            sr.run(lengths, rec, 3, clear)
        assert e.value.code == -4, what
    with pytest.raises(SrError) as e:
        sr.run([1 << 21], np.zeros(0, dtype=REC))
    assert e.value.code == -4
    with pytest.raises(SR.BadInput):
        SR.split_reads([1 << 21], np.zeros(0, dtype=REC), 3, None, SR.Params())
    check(sr, lengths, good)                            # and the context still works
    check(sr, lengths, good, clear=([0, U32, 0], [2000, U32, 2000]))


# ------------------------------------------------------------------ the chain

@pytest.mark.parametrize("clear_on_device", [False, True])
def test_chain_from_the_overlapper(sr, clear_on_device):
    """OverlapInCore.run -> store_view -> TrimReads.run -> SplitReads.run, no file in between,
    the records in HBM; in the second variant the clear ranges too."""
    import torch
    from canu_amd.find_errors import store_view
    from canu_amd.overlap_in_core import OicParameters, OverlapInCore
    from canu_amd.split_reads import SrParameters
    from canu_amd.synth import synth_reads
    from canu_amd.trim_reads import TrimReads, TrParameters
    rs = synth_reads(n_reads=60, read_len=1500, genome_len=12_000, error_rate=0.01, seed=21)
    P = OicParameters(Kmer_Len=22, maxErate=float(np.float32(0.06)), Min_Olap_Len=100,
                      Doing_Partial_Overlaps=True).finalize()
    oic = OverlapInCore(P, device=0)
    view = store_view(oic.run(rs))
    oic.close()
    assert view.shape[0] > 100
    tr = TrimReads(TrParameters(erate=0.03, min_read_length=500, min_evidence_coverage=2))
    trimmed = tr.run(rs.lengths, view)
    tr.close()
    cb, ce = trimmed.clear_ranges()
    assert ((cb > 0) & (cb != U32)).any()                # trimReads cut something
    d_rec = torch.from_numpy(view.view(np.uint8).reshape(-1).copy()).cuda()
    P2 = SrParameters(min_read_length=500)
    sr.set_params(P2)
    if clear_on_device:
        d_cb = torch.from_numpy(cb.astype(np.int32)).cuda()
        d_ce = torch.from_numpy(ce.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        got = sr.run(rs.lengths, view, 3, device_records=d_rec.data_ptr(), n_device_records=view.shape[0],
                     device_clear=(d_cb.data_ptr(), d_ce.data_ptr()))
    else:
        torch.cuda.synchronize()
        got = sr.run(rs.lengths, view, 3, clear=trimmed, device_records=d_rec.data_ptr(),
                     n_device_records=view.shape[0])
    rp = SR.Params(P2.erate, P2.min_read_length)
    want = SR.split_reads(rs.lengths, view, 3, (cb, ce), rp)
    compare(got, want, rp, view)
    assert got.stats["n_overlaps"] > 0 and (want["n_adjusted"] > 0).any()
