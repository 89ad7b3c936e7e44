#!/usr/bin/env python3
"""Measure the GPU trimReads (canu_amd.trim_reads, libcanu_tr.so) on one GPU.

    python bench_tr.py [--reads 1000000] [--steps 5] [--warmup 1]

The workload is the synthetic store of fixed seed of canu_amd.trim_reads.synth_store_view: reads
of 500 .. 3000 bases, a skewed (log-normal) number of overlaps per read, three reads beyond the
wave's capacity, every overlap with its twin as an overlap store holds them.  The records are
put into device memory once (as `OverlapInCore.run` leaves them there in the chain); a step is
one `TrimReads.run` over all reads, best of --steps.  One JSON line: reads/s and overlaps/s of
the whole call, the ms of each kernel group, the algorithmic bytes (24 per record in, 4 per
length, 18 per read out) over the kernels' time as a fraction of the HBM peak, the time of one
call with the records on the host, and a parity block: sampled reads against the Python
restatement of the reference (tests/tr_restate.py).  tools/make_tr_golden.py --time runs the
reference program on the same store.  No threshold is set here: the line is a measurement.
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
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--coverage", type=int, default=1)
    ap.add_argument("--parity-reads", type=int, default=300)
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_tr.py: trimReads runs on one GPU")
    import numpy as np
    from canu_amd.trim_reads import TrimReads, TrParameters, synth_store_view, wave_capacity
    lens, rec = synth_store_view(a.reads, a.seed)
    import torch  # torch's HIP runtime first, as in bench.py and the tests
    import tr_restate as TR

    P = TrParameters(min_evidence_coverage=a.coverage)
    tr = TrimReads(P)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    best, res = None, None
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = tr.run(lens, None, 1, device_records=d_rec.data_ptr(), n_device_records=rec.shape[0])
        dt = time.perf_counter() - t0
        if step >= a.warmup and (best is None or dt < best):
            best, res = dt, r
    t0 = time.perf_counter()
    host = tr.run(lens, rec, 1)
    t_host = time.perf_counter() - t0
    tr.close()
    same = all(np.array_equal(getattr(host, k), getattr(res, k)) for k in ("bgn", "end", "status", "flags"))

    # parity: the largest reads, the large-path reads and a random sample, restated
    cnt = np.bincount(rec["a"], minlength=a.reads + 1)[1:]
    rng = np.random.default_rng(1)
    pick = np.unique(np.concatenate([np.argsort(cnt)[-8:], rng.choice(a.reads, min(a.parity_reads, a.reads),
                                                                      replace=False)])) + 1
    off = np.searchsorted(rec["a"], np.arange(1, a.reads + 2))
    sub_len = lens[pick - 1]
    parts, bad = [], 0
    for k, rid in enumerate(pick):
        part = rec[off[rid - 1]:off[rid]].copy()
        part["a"] = k + 1
        parts.append(part)
    want = TR.trim_reads(sub_len, np.concatenate(parts), 1,
                         TR.Params(P.erate, P.min_read_length, P.min_evidence_overlap, P.min_evidence_coverage))
    for k, rid in enumerate(pick):
        i = rid - 1
        bad += not (want["bgn"][k] == res.bgn[i] and want["end"][k] == res.end[i] and
                    want["status"][k] == res.status[i] and want["n_used"][k] == res.n_used[i])

    s = res.stats
    kernel_s = (s["ms_segment"] + s["ms_wave"] + s["ms_large"]) / 1e3
    algo_bytes = 24 * rec.shape[0] + 4 * a.reads + 18 * a.reads
    line = {
        "bench": "trimReads", "reads": a.reads, "overlaps": int(rec.shape[0]),
        "wave_capacity": wave_capacity(), "min_evidence_coverage": a.coverage,
        "seconds": round(best, 6), "reads_per_s": round(a.reads / best, 1),
        "overlaps_per_s": round(rec.shape[0] / best, 1),
        "ms_segment": round(s["ms_segment"], 3), "ms_wave": round(s["ms_wave"], 3),
        "ms_large": round(s["ms_large"], 3),
        "n_wave_reads": s["n_wave_reads"], "n_large_reads": s["n_large_reads"], "n_literal": s["n_literal"],
        "max_overlaps_of_a_read": int(cnt.max()),
        "algorithmic_bytes": algo_bytes,
        "kernel_bytes_per_s": round(algo_bytes / kernel_s, 1) if kernel_s else None,
        "fraction_of_hbm_peak": round(algo_bytes / kernel_s / HBM_PEAK, 5) if kernel_s else None,
        "seconds_records_on_host": round(t_host, 6),
        "status_counts": {TR.TAGS[k]: int((res.status == k).sum()) for k in TR.TAGS},
        "parity": {"reads_checked": int(pick.shape[0]), "mismatches": int(bad),
                   "host_records_equal_device_records": bool(same)},
        "steps": a.steps, "warmup": a.warmup,
    }
    print(json.dumps(line), flush=True)
    if bad or not same:
        raise SystemExit("bench_tr.py: the GPU result differs from the restatement")


if __name__ == "__main__":
    main()
