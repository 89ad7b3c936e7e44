#!/usr/bin/env python3
"""Measure the GPU splitReads (canu_amd.split_reads, libcanu_sr.so) on one GPU.

    python bench_sr.py [--reads 200000] [--steps 5] [--warmup 1]

The workload is the synthetic store of fixed seed of canu_amd.split_reads.synth_store_view: the
reads and overlaps of bench_tr.py's store, every overlap with its twin as an overlap store holds
them, and on one read in twenty a planted subread junction (four to eight twin pairs).  The
records are put into device memory once (as `OverlapInCore.run` leaves them there in the chain);
a step is one `SplitReads.run` over all reads, best of --steps.  One JSON line: reads/s and
overlaps/s of the whole call, the ms of each kernel group, the algorithmic bytes (24 per record
in, 9 per read in, 16 per read and 1 per record out) over the kernels' time as a fraction of the
HBM peak, the time of one call with the records on the host, and a parity block: sampled reads
against the Python restatement of the reference (tests/sr_restate.py).
tools/make_sr_golden.py --time runs the reference program on the same store.  No threshold is set
here: the line is a measurement.
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

HBM_PEAK = 8.0e12                       # bytes/s, MI355X


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--parity-reads", type=int, default=300)
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_sr.py: splitReads runs on one GPU")
    import numpy as np
    from canu_amd.split_reads import SplitReads, SrParameters, synth_store_view, wave_capacity
    lens, rec = synth_store_view(a.reads, a.seed)
    import torch  # torch's HIP runtime first, as in bench.py and the tests
    import sr_restate as SR

    P = SrParameters()
    sr = SplitReads(P)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    best, res = None, None
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = sr.run(lens, None, 3, device_records=d_rec.data_ptr(), n_device_records=rec.shape[0])
        dt = time.perf_counter() - t0
        if step >= a.warmup and (best is None or dt < best):
            best, res = dt, r
    t0 = time.perf_counter()
    host = sr.run(lens, rec, 3)
    t_host = time.perf_counter() - t0
    sr.close()
    same = all(np.array_equal(getattr(host, k), getattr(res, k))
               for k in ("bgn", "end", "status", "fate", "n_adjusted", "n_bad_regions", "regions"))

    # parity: the largest reads, the trimmed reads and a random sample, restated.  A read's
    # result needs its own records and its partners' lengths only (no clear ranges here).
    cnt = np.bincount(rec["a"], minlength=a.reads + 1)[1:]
    rng = np.random.default_rng(1)
    hit = np.flatnonzero(res.n_bad_regions > 0)
    pick = np.unique(np.concatenate([np.argsort(cnt)[-8:], hit[:a.parity_reads],
                                     rng.choice(a.reads, min(a.parity_reads, a.reads), replace=False)])) + 1
    off = np.searchsorted(rec["a"], np.arange(1, a.reads + 2))
    keep = np.zeros(rec.shape[0], bool)
    for rid in pick:
        keep[off[rid - 1]:off[rid]] = True
    want = SR.split_reads(lens, rec[keep], 3, None, SR.Params(P.erate, P.min_read_length))
    i = pick - 1
    bad = int(((want["bgn"][i] != res.bgn[i]) | (want["end"][i] != res.end[i]) | (want["status"][i] != res.status[i]) |
               (want["n_adjusted"][i] != res.n_adjusted[i]) | (want["n_bad_regions"][i] != res.n_bad_regions[i])).sum())
    bad += int(not np.array_equal(want["fate"], res.fate[keep]))
    picked = set(int(v) for v in pick)
    bad += int([tuple(int(v) for v in g) for g in res.regions if int(g["read"]) in picked] != want["regions"])

    s = res.stats
    kernel_s = (s["ms_records"] + s["ms_wave"] + s["ms_large"]) / 1e3
    algo_bytes = 24 * rec.shape[0] + 9 * a.reads + 16 * a.reads + rec.shape[0]
    line = {
        "bench": "splitReads", "reads": a.reads, "overlaps": int(rec.shape[0]),
        "wave_capacity": wave_capacity(),
        "seconds": round(best, 6), "reads_per_s": round(a.reads / best, 1),
        "overlaps_per_s": round(rec.shape[0] / best, 1),
        "ms_records": round(s["ms_records"], 3), "ms_wave": round(s["ms_wave"], 3),
        "ms_large": round(s["ms_large"], 3),
        "n_wave_reads": s["n_wave_reads"], "n_large_reads": s["n_large_reads"], "n_regions": s["n_regions"],
        "max_overlaps_of_a_read": int(cnt.max()),
        "algorithmic_bytes": algo_bytes,
        "kernel_bytes_per_s": round(algo_bytes / kernel_s, 1) if kernel_s else None,
        "fraction_of_hbm_peak": round(algo_bytes / kernel_s / HBM_PEAK, 5) if kernel_s else None,
        "seconds_records_on_host": round(t_host, 6),
        "status_counts": {str(k): int((res.status == k).sum()) for k in range(8)},
        "error_lines": int((res.fate >= 3).sum()),
        "parity": {"reads_checked": int(pick.shape[0]), "mismatches": int(bad),
                   "host_records_equal_device_records": bool(same)},
        "steps": a.steps, "warmup": a.warmup,
    }
    print(json.dumps(line), flush=True)
    if bad or not same:
        raise SystemExit("bench_sr.py: the GPU result differs from the restatement")


if __name__ == "__main__":
    main()
