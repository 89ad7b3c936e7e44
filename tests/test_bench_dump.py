"""bench.py --dump-outputs (CPU): the dump is the last step's records in ovStore order, every
value exact in a double, whatever order the job handed them back in; and --full is what
switches on the figures beside the headline."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


class _FakeOic:
    def __init__(self, rec):
        self.rec = rec

    def fetch(self):
        return self.rec


def _records(n, seed):
    from canu_amd.digest import RECORD_DTYPE
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=RECORD_DTYPE)
    rec["a"] = rng.integers(1, 50, n)
    rec["b"] = rng.integers(1, 2**32 - 1, n, dtype=np.uint64)
    rec["w0"] = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    rec["w1"] = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    return rec


def test_dump_is_sorted_exact_and_order_independent(tmp_path):
    import bench
    from canu_amd.digest import sort_records
    rec = _records(1000, 7)
    st = {k: i + 1 for i, k in enumerate(bench.DUMP_COUNTERS)}
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), _FakeOic(rec), st, 0, 1)
    bench.dump_outputs(str(b), _FakeOic(rec[np.random.default_rng(1).permutation(1000)]),
                       st, 0, 1)
    assert info == {"records": 1000, "rows_written": 1000}
    rows = np.load(a / "records.npy")
    assert rows.dtype == np.float64 and rows.shape == (1000, 6)
    assert np.array_equal(rows, np.load(b / "records.npy"))
    want = sort_records(rec)
    assert np.array_equal(rows[:, 0].astype(np.uint32), want["a"])
    assert np.array_equal(rows[:, 1].astype(np.uint32), want["b"])
    u = rows[:, 2:].astype(np.uint64)
    assert np.array_equal(u[:, 0] | (u[:, 1] << np.uint64(32)), want["w0"])
    assert np.array_equal(u[:, 2] | (u[:, 3] << np.uint64(32)), want["w1"])
    counters = np.load(a / "counters.npy")
    assert counters.dtype == np.float64
    assert counters.tolist() == [float(i + 1) for i in range(len(bench.DUMP_COUNTERS))] + [1000.0]


def test_dump_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 48 * 100)
    rec = _records(1000, 9)
    st = dict.fromkeys(bench.DUMP_COUNTERS, 0)
    info = bench.dump_outputs(str(tmp_path / "a"), _FakeOic(rec), st, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), _FakeOic(rec[::-1].copy()), st, 0, 1)
    assert info == {"records": 1000, "rows_written": 100}
    rows = np.load(tmp_path / "a" / "records.npy")
    assert rows.shape == (100, 6)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "records.npy"))
    assert np.load(tmp_path / "a" / "counters.npy")[-1] == 1000.0


class _SpyOic:
    """Counts the kernel runs a roofline asks for."""

    def __init__(self):
        self.calls = []

    def probe_ceiling(self):
        self.calls.append("probe_ceiling")
        return 50.0, 1 << 30

    def probe_replay(self, lo, hi):
        self.calls.append("probe_replay")
        return 48.0, 1000

    def close(self):
        self.calls.append("close")


class _SpyJob:
    """A finished job whose side measurements only record that they were asked for."""
    n, nloaded, total_bases, q_lo, q_hi = 100, 100, 1_000_000, 1, 100

    def __init__(self, args):
        self.args, self.oic, self.calls = args, _SpyOic(), []

    def workload_key(self):
        return {"workload": "none of the profiled ones"}

    def _note(name):
        def f(self, *a, **k):
            self.calls.append(name)
            return {"from": name}
        return f

    parity, seed_only, shard_timing = _note("parity"), _note("seed_only"), _note("shard_timing")
    index_allgather_timing, write_output = _note("index_allgather"), _note("write_output")
    release = _note("release")


_STATS = {"pairs": 10, "seed_nodes": 100, "total_overlaps": 9, "extend_launches": 1,
          "ms_extend": 2.0, "probe_launches": 1, "ms_probe_kernel": 1.0, "probe_bytes": 1 << 20,
          "probe_sorted_launches": 0}


class _NoTorch:
    class cuda:
        @staticmethod
        def empty_cache():
            pass


def _after_timing(monkeypatch, argv, world=1):
    import bench
    ran = []
    monkeypatch.setattr(bench, "cpu_baseline", lambda args: ran.append("cpu_baseline") or {})
    monkeypatch.setattr(bench, "side_runs", lambda: ran.append("side_runs") or {"side": 1})
    monkeypatch.setenv("CANU_DEVICE", "0")
    job = _SpyJob(bench.parse_args(argv))
    out = bench.after_timing(job.args, job, _STATS, 0, world, "gloo", 1.0, None, None, _NoTorch)
    return out, job.calls + job.oic.calls + ran


def test_plain_run_measures_nothing_beside_the_headline(monkeypatch):
    for world in (1, 2):
        out, calls = _after_timing(monkeypatch, ["--gpus", str(world), "--steps", "2"], world)
        assert calls == []
        roof, probe_roof, _ = out.pop("rooflines")
        assert roof["kernel"] == "k_extend" and probe_roof["kernel"] == "k_probe"
        assert probe_roof["random_lookup_ceiling"] is None
        assert set(out) == {"parity", "ovb", "seed_only", "shard_timing", "xgmi", "cpu", "side"}
        assert all(v is None for v in out.values())


def test_full_run_measures_everything_and_keeps_the_switches(monkeypatch):
    out, calls = _after_timing(monkeypatch, ["--full"])
    assert calls == ["parity", "seed_only", "shard_timing", "release", "probe_ceiling",
                     "probe_replay", "close", "cpu_baseline", "side_runs"]
    assert out["rooflines"][1]["random_lookup_ceiling"]["ceiling_gloads_per_s"] == 50.0
    assert out["parity"] and out["seed_only"] and out["shard_timing"] and out["side"]
    out, calls = _after_timing(monkeypatch, ["--full"], world=2)
    assert calls == ["parity", "index_allgather", "probe_ceiling", "probe_replay"]
    out, calls = _after_timing(monkeypatch, ["--full", "--no-parity", "--no-seed-only",
                                             "--no-shard-timing", "--no-cpu-baseline",
                                             "--no-side"])
    assert calls == ["probe_ceiling", "probe_replay"]
    # an explicit --ovb-out is honoured in either mode
    out, calls = _after_timing(monkeypatch, ["--ovb-out", "d"])
    assert calls == ["write_output"] and out["ovb"] == {"from": "write_output"}


def test_configs4_side_line_is_a_full_run_of_its_own(monkeypatch):
    import subprocess
    import bench
    cmds = []

    class _Done:
        returncode, stdout, stderr = 0, '{"value": 1.0, "parity": {"ok": true}}\n', ""

    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: cmds.append(cmd) or _Done)
    out = bench.side_runs()
    c4 = [c for c in cmds if c[1].endswith("bench.py")]
    assert len(c4) == 1 and "--full" in c4[0] and "--no-side" in c4[0]
    assert out["configs4_rank"]["parity"] == {"ok": True}


def test_plain_and_full_arguments():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
