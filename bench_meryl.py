#!/usr/bin/env python3
"""Measure the GPU k-mer count (canu_amd.meryl, libcanu_meryl.so) on one GPU.

    python bench_meryl.py [--k 22] [--reads 50000] [--read-len 10000] [--steps 3] [--warmup 1]

The read set is bench.py's flagship one (50k x 10 kb at 25x, 1.5 % error, seed 1); --k 16 is
MHAP's mer size.  One JSON line: mers/s over the timed counts, the per-phase device ms of the
last one, the passes, each phase's algorithmic bytes and their fraction of the 8 TB/s HBM peak,
and a parity block that compares totals and histogram of a 2,000-read subsample with the numpy
restatement (tests/meryl_numpy.py).  No threshold is set here: the line is a measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_BYTES_PER_S = 8.0e12


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", type=int, default=22)
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=float, default=25.0)
    ap.add_argument("--read-error", type=float, default=0.015)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--low-count", type=int, default=2)
    ap.add_argument("--hbm-budget", type=int, default=0, help="bytes; 0 = the library's default")
    ap.add_argument("--parity-reads", type=int, default=2000)
    ap.add_argument("--fasta-out", default=None,
                    help="also write the read set as FASTA (input of a CPU baseline run)")
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_meryl.py: the count runs on one GPU (multi-GPU is out of scope)")
    import numpy as np
    from canu_amd.synth import ReadSet, synth_reads_parallel
    # generated before anything touches the GPU (no pool is forked from a GPU process)
    rs = synth_reads_parallel(a.reads, a.read_len, int(a.reads * a.read_len / a.coverage),
                              a.read_error, seed=a.seed, workers=16)
    if a.fasta_out:
        with open(a.fasta_out, "wb") as f:
            for i in range(rs.nreads):
                f.write(b">r%d\n" % i + rs.read(i) + b"\n")
    import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py and the tests)
    import meryl_numpy as MN
    from canu_amd import meryl

    mc = meryl.MerCounter(a.k, True, a.low_count, hbm_budget=a.hbm_budget or None)
    t0 = time.perf_counter()
    mc.load_reads(rs)
    load_s = time.perf_counter() - t0
    for _ in range(a.warmup):
        mc.count()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        mc.count()
        times.append(time.perf_counter() - t0)
    st = mc.stats()
    mc.close()

    total, kept, packed = st["total_mers"], st["kept_mers"], st["packed_read_bytes"]
    phases = {
        # the packed reads once per planner scan
        "emit": {"ms": st["ms_plan"], "bytes": st["plan_scans"] * packed},
        # per pass the reads twice (bucket sizes, then the scatter); 8 B written per mer
        "partition": {"ms": st["ms_partition"], "bytes": 2 * st["passes"] * packed + 8 * total},
        # 8 B read per mer at the fine sort, 12 B out per kept distinct mer
        "sort_reduce": {"ms": st["ms_sort"], "bytes": 8 * total + 12 * kept},
    }
    for p in phases.values():
        p["hbm_fraction"] = (p["bytes"] / (p["ms"] * 1e-3) / HBM_PEAK_BYTES_PER_S) if p["ms"] else 0.0

    n = min(a.parity_reads, rs.nreads)
    end = int(rs.offsets[n - 1]) + int(rs.lengths[n - 1])
    sub = ReadSet(bases=rs.bases[:end], offsets=rs.offsets[:n], lengths=rs.lengths[:n])
    want = MN.count_reads(sub, a.k, True, a.low_count)
    ms = meryl.MerCounter(a.k, True, a.low_count)
    ms.load_reads(sub)
    ms.count()
    s2 = ms.stats()
    parity = {"reads": n,
              "totals": (s2["total_mers"], s2["distinct_mers"], s2["unique_mers"],
                         s2["largest_count"]) == (want.total, want.distinct, want.unique,
                                                  want.largest),
              "histogram": bool(np.array_equal(ms.histogram(), want.hist)),
              "kept": all(np.array_equal(x, y) for x, y in zip(ms.frequent(0), want.frequent(0)))}
    parity["ok"] = parity["totals"] and parity["histogram"] and parity["kept"]
    ms.close()

    best = min(times)
    line = {"bench": "meryl", "k": a.k, "reads": a.reads, "read_len": a.read_len,
            "coverage": a.coverage, "low_count": a.low_count,
            "total_mers": total, "distinct_mers": st["distinct_mers"],
            "unique_mers": st["unique_mers"], "kept_mers": kept,
            "count_s": best, "count_s_all": times, "mers_per_s": total / best,
            "load_s": load_s, "passes": st["passes"], "plan_scans": st["plan_scans"],
            "oversize_buckets": st["oversize_buckets"], "budget_bytes": st["budget_bytes"],
            "peak_device_bytes": st["peak_device_bytes"], "packed_read_bytes": packed,
            "device_ms": st["ms_plan"] + st["ms_partition"] + st["ms_sort"],
            "phases": phases, "parity": parity}
    print(json.dumps(line), flush=True)
    if not parity["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
