#!/usr/bin/env python3
"""Measure the GPU overlapPair (canu_amd.pair, libcanu_pair.so) on one GPU.

    python bench_pair.py [--reads 2000] [--read-len 15000] [--overlaps 20000] [--steps 3]

The reads have the configs[3] shape (15 kb at 25x); the input overlaps are the reads' true
overlaps with each hang moved by up to +-300 bases, as MHAP reports them, so no MHAP run is
needed.  Two JSON lines: `cor` (-partial, erate 0.30, reads at 5 % error) and `utg` (erate
0.045, reads at 1 % error), each with overlaps/s, DP cells/s (query rows x target columns of
every pass), the kernel's ms, its VALU issue fraction (wavefront steps x the step loop's VALU
count from the ISA, against 1,024 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction) and a
parity block: a sample of the output against the Python restatement of the reference
(tests/pair_restate.py; the whole set would take it hours).  No threshold is set here: the
lines are measurements.
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

VALU_ISSUE_PEAK_G = 256 * 4 * 2.4 / 2.0     # G wave64 VALU instructions/s (bench_mhap.py)
VALU_PER_STEP = 102                         # k_pair's step loop, counted in the gfx950 ISA
MODES = {"cor": dict(partial=True, erate=0.30, read_error=0.05),
         "utg": dict(partial=False, erate=0.045, read_error=0.01)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=15_000)
    ap.add_argument("--coverage", type=float, default=25.0)
    ap.add_argument("--overlaps", type=int, default=20_000)
    ap.add_argument("--min-len", type=int, default=500)
    ap.add_argument("--jitter", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--modes", default="cor,utg")
    ap.add_argument("--parity-overlaps", type=int, default=12)
    ap.add_argument("--dump-dir", default=None,
                    help="also write reads.bin / in.ovb per mode (inputs of a CPU baseline run)")
    return ap.parse_args(argv)


def true_overlaps(rs, n_want: int, jitter: int, seed: int, min_true: int = 2000):
    """ovOverlap records of read pairs that share at least min_true genome bases, hangs from
    the reads' genome positions, each moved by up to +-jitter."""
    import numpy as np
    from canu_amd.overlap_in_core import RECORD_DTYPE
    rng = np.random.default_rng([seed, 77])
    lens = rs.lengths.astype(np.int64)
    s, e = rs.starts.astype(np.int64), rs.starts.astype(np.int64) + lens
    order = np.argsort(s, kind="stable")
    pairs = []
    for ii, i in enumerate(order):
        for j in order[ii + 1:]:
            if s[j] > e[i] - min_true:
                break
            if min(e[i], e[j]) - s[j] >= min_true:
                pairs.append((int(min(i, j)), int(max(i, j))))
    pairs = np.array(pairs, dtype=np.int64)
    if pairs.shape[0] > n_want:
        pairs = pairs[np.sort(rng.choice(pairs.shape[0], n_want, replace=False))]
    a, b = pairs[:, 0], pairs[:, 1]
    lo, hi = np.maximum(s[a], s[b]), np.minimum(e[a], e[b])
    fwd = rs.strands[a] == 0
    a5 = np.where(fwd, lo - s[a], e[a] - hi)
    a3 = np.where(fwd, e[a] - hi, lo - s[a])
    b5 = np.where(fwd, lo - s[b], e[b] - hi)
    b3 = np.where(fwd, e[b] - hi, lo - s[b])
    jit = rng.integers(-jitter, jitter + 1, size=(4, a.shape[0]))
    a5 = np.clip(a5 + jit[0], 0, lens[a] - 1)
    a3 = np.clip(a3 + jit[1], 0, lens[a] - 1 - a5)
    b5 = np.clip(b5 + jit[2], 0, lens[b] - 1)
    b3 = np.clip(b3 + jit[3], 0, lens[b] - 1 - b5)
    flipped = (rs.strands[a] != rs.strands[b]).astype(np.uint64)
    rec = np.zeros(a.shape[0], dtype=RECORD_DTYPE)
    rec["a"], rec["b"] = a + rs.first_iid, b + rs.first_iid
    rec["w0"] = a5.astype(np.uint64) | (a3.astype(np.uint64) << np.uint64(21)) | \
        (flipped << np.uint64(54))
    rec["w1"] = b5.astype(np.uint64) | (b3.astype(np.uint64) << np.uint64(21))
    return rec


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_pair.py: overlapPair runs on one GPU")
    import numpy as np
    from canu_amd.synth import synth_reads_parallel, write_reads_file
    # generated before anything touches the GPU (no pool is forked from a GPU process)
    work = {}
    for mode in a.modes.split(","):
        M = MODES[mode]
        rs = synth_reads_parallel(a.reads, a.read_len, int(a.reads * a.read_len / a.coverage),
                                  M["read_error"], seed=a.seed, workers=16)
        work[mode] = (rs, true_overlaps(rs, a.overlaps, a.jitter, a.seed))
    import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py and the tests)
    import pair_restate as PR
    from canu_amd import pair
    from canu_amd.overlap_in_core import write_ovb

    ok = True
    for mode, (rs, recs) in work.items():
        M = MODES[mode]
        if a.dump_dir:
            os.makedirs(a.dump_dir, exist_ok=True)
            write_reads_file(os.path.join(a.dump_dir, f"{mode}.reads.bin"), rs)
            write_ovb(recs, os.path.join(a.dump_dir, f"{mode}.in.ovb"), counts=False)
        P = pair.PairParameters(M["erate"], a.min_len, M["partial"], False)
        op = pair.OverlapPair(P)
        t0 = time.perf_counter()
        op.load_reads(rs)
        load_s = time.perf_counter() - t0
        for _ in range(a.warmup):
            op.realign(recs)
        times, kms = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            out = op.realign(recs)
            times.append(time.perf_counter() - t0)
            kms.append(op.stats()["ms_kernel"])
        st, counters = op.stats(), op.counters()
        op.close()

        n_par = min(a.parity_overlaps, recs.shape[0])
        pick = np.linspace(0, recs.shape[0] - 1, n_par).astype(np.int64) if n_par else []
        reads = {}
        for r in recs[pick]:
            for iid in (int(r["a"]), int(r["b"])):
                reads[iid] = rs.read(iid - rs.first_iid)
        want, _ = PR.realign(recs[pick], reads, M["erate"], a.min_len, M["partial"], False)
        parity = {"overlaps": int(n_par), "of": int(recs.shape[0]),
                  "ok": bool(np.array_equal(out[pick], want))}
        ok &= parity["ok"]

        best, k_ms = min(times), min(kms)
        valu_g = st["dp_steps"] * VALU_PER_STEP / (k_ms * 1e-3) / 1e9
        line = {"bench": "overlapPair", "mode": mode, "reads": a.reads, "read_len": a.read_len,
                "read_error": M["read_error"], "erate": M["erate"], "partial": M["partial"],
                "min_len": a.min_len, "overlaps": int(recs.shape[0]), "banded": False,
                "realign_s": best, "realign_s_all": times, "kernel_ms": k_ms,
                "overlaps_per_s": recs.shape[0] / best,
                "kernel_overlaps_per_s": recs.shape[0] / (k_ms * 1e-3),
                "dp_cells": st["dp_cells"], "dp_passes": st["dp_passes"],
                "dp_steps": st["dp_steps"], "g_cells_per_s": st["dp_cells"] / (k_ms * 1e-3) / 1e9,
                "valu_per_step": VALU_PER_STEP,
                "valu_lane_ops_per_cell": VALU_PER_STEP * st["dp_steps"] * 64.0 / max(st["dp_cells"], 1),
                "valu_issue": {"achieved": round(valu_g, 1), "peak": VALU_ISSUE_PEAK_G,
                               "unit": "G VALU wave-instructions/s",
                               "frac": round(valu_g / VALU_ISSUE_PEAK_G, 4)},
                "load_s": load_s, "counters": counters, "parity": parity}
        print(json.dumps(line), flush=True)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
