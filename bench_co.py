#!/usr/bin/env python3
"""Measure the GPU correctOverlaps (canu_amd.correct_overlaps, libcanu_co.so) on one GPU.

    python bench_co.py [--reads 2000] [--read-len 12000] [--steps 3] [--dump-dir DIR]

The reads are bench_fe.py's (12 kb at 25x by default, 1 % error); the overlaps are
`OverlapInCore.run`'s through `store_view`, and the corrections are `FindErrors.run`'s over all
reads, so the job is the second half of overlap error adjustment on what the first half gave.
One JSON line: overlaps/s, edit-distance rows/s, aligned bases/s (the sum of min(a_part, b_part)
over the overlaps), the ms of each kernel, the counters, k_fe_align's time on the same reads
and overlaps as the nearest yardstick, and a parity block: the evalues of a sample of reads'
overlaps against the Python restatement of the reference (tests/co_restate.py).  No threshold
is set here: the line is a measurement.
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=12_000)
    ap.add_argument("--coverage", type=float, default=25.0)
    ap.add_argument("--read-error", type=float, default=0.01)
    ap.add_argument("--erate", type=float, default=0.045)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parity-reads", type=int, default=3)
    ap.add_argument("--dump-dir", default=None,
                    help="also write reads.bin / in.ovb / gpu.red (inputs of a CPU baseline run) "
                         "and gpu.oea")
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_co.py: correctOverlaps runs on one GPU")
    import numpy as np
    from canu_amd.synth import synth_reads_parallel, write_reads_file
    # generated before anything touches the GPU (no pool is forked from a GPU process)
    rs = synth_reads_parallel(a.reads, a.read_len, int(a.reads * a.read_len / a.coverage),
                              a.read_error, seed=a.seed, workers=16)
    import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py and the tests)
    import co_restate as CR
    from canu_amd import correct_overlaps as CO
    from canu_amd import find_errors as FE
    from canu_amd.overlap_in_core import OicParameters, OverlapInCore, write_ovb

    P = OicParameters(Kmer_Len=22, maxErate=float(np.float32(a.erate)), Min_Olap_Len=500).finalize()
    oic = OverlapInCore(P, device=0)
    t0 = time.perf_counter()
    ovl = oic.run(rs)
    oic_s = time.perf_counter() - t0
    oic.close()
    store = FE.store_view(ovl)
    bgn, end = rs.first_iid, rs.first_iid + rs.nreads - 1

    fe = FE.FindErrors(FE.FeParameters(error_rate=a.erate))
    fe.load_reads(rs)
    fe.run(store, bgn, end)                               # warm, then the timed one
    t0 = time.perf_counter()
    red = fe.run(store, bgn, end)
    fe_s = time.perf_counter() - t0
    fe_st = fe.stats()
    if a.dump_dir:
        os.makedirs(a.dump_dir, exist_ok=True)
        write_reads_file(os.path.join(a.dump_dir, "reads.bin"), rs)
        write_ovb(ovl, os.path.join(a.dump_dir, "in.ovb"), counts=False)
        fe.write_red(os.path.join(a.dump_dir, "gpu.red"))
    fe.close()

    co = CO.CorrectOverlaps(CO.CoParameters(error_rate=a.erate))
    t0 = time.perf_counter()
    co.load_reads(rs)
    load_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    co.set_corrections(red)
    correct_s = time.perf_counter() - t0
    for _ in range(a.warmup):
        co.run(store, bgn, end)
    times, stats = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        out = co.run(store, bgn, end)
        times.append(time.perf_counter() - t0)
        stats.append(co.stats())
    counters = co.counters()
    if a.dump_dir:
        co.write_oea(os.path.join(a.dump_dir, "gpu.oea"))
    co.close()
    k = int(np.argmin(times))
    best, st = times[k], stats[k]

    # parity: a few reads' overlaps, each read as a range of its own
    pick = [int(v) for v in np.linspace(bgn, end, a.parity_reads).astype(np.int64)]
    ok = True
    n_par = 0
    for rid in pick:
        at = np.nonzero(store["a"] == rid)[0]
        sel = store[at]
        n_par += int(sel.shape[0])
        reads = {rid: rs.read(rid - rs.first_iid)}
        for b in sel["b"]:
            reads[int(b)] = rs.read(int(b) - rs.first_iid)
        want, _ = CR.correct_overlaps(sel, reads, red, rid, rid, a.erate)
        ok &= bool(np.array_equal(out[at], want))

    came = CO.evalues_of(store)
    ms = st["ms_align"]
    line = {"bench": "correctOverlaps", "reads": a.reads, "read_len": a.read_len,
            "read_error": a.read_error, "erate": a.erate, "overlaps": int(store.shape[0]),
            "corrections": int(red.shape[0]) - rs.nreads,
            "correct_overlaps_s": best, "correct_overlaps_s_all": times,
            "overlaps_per_s": store.shape[0] / best,
            "aligned_bases": st["bases"], "g_aligned_bases_per_s": st["bases"] / best / 1e9,
            "rows": st["rows"], "m_rows_per_s": st["rows"] / best / 1e6,
            "kernel_ms": {"k_co_correct": st["ms_correct"], "k_co_align": ms},
            "kernel_overlaps_per_s": store.shape[0] / (ms * 1e-3) if ms else None,
            "generic_alignments": st["n_generic"], "staged_alignments": st["n_staged"],
            "regrows": st["regrows"], "scratch_bytes": st["scratch_bytes"],
            "load_s": load_s, "set_corrections_s": correct_s, "overlapper_s": oic_s,
            "evalues": {"lowered": int((out < came).sum()), "raised": int((out > came).sum()),
                        "same": int((out == came).sum())},
            "counters": counters,
            "find_errors": {"find_errors_s": fe_s, "k_fe_align_ms": fe_st["ms_align"],
                            "rows": fe_st["rows"], "aligned_bases": fe_st["bases"]},
            "parity": {"reads": pick, "overlaps": n_par, "of": int(store.shape[0]), "ok": ok}}
    print(json.dumps(line), flush=True)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
