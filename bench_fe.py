#!/usr/bin/env python3
"""Measure the GPU findErrors (canu_amd.find_errors, libcanu_fe.so) on one GPU.

    python bench_fe.py [--reads 2000] [--read-len 12000] [--steps 3] [--dump-dir DIR]

The reads have bench.py's shape (12 kb at 25x by default) at utg-like error (1 %); the overlaps
are `OverlapInCore.run`'s through `store_view`, so both reads of each pair see the overlap, as
in a store.  One JSON line: overlaps/s, aligned bases/s (the sum of min(a_part, b_part) over the
overlaps), edit-distance rows/s, the ms of each kernel, and a parity block: the records of a
sample of reads against the Python restatement of the reference (tests/fe_restate.py) on those
reads' overlaps.  No threshold is set here: the line is a measurement.
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
                    help="also write reads.bin / in.ovb (inputs of a CPU baseline run) and gpu.red")
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_fe.py: findErrors runs on one GPU")
    import numpy as np
    from canu_amd.synth import synth_reads_parallel, write_reads_file
    # generated before anything touches the GPU (no pool is forked from a GPU process)
    rs = synth_reads_parallel(a.reads, a.read_len, int(a.reads * a.read_len / a.coverage),
                              a.read_error, seed=a.seed, workers=16)
    import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py and the tests)
    import fe_restate as FR
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
    if a.dump_dir:
        os.makedirs(a.dump_dir, exist_ok=True)
        write_reads_file(os.path.join(a.dump_dir, "reads.bin"), rs)
        write_ovb(ovl, os.path.join(a.dump_dir, "in.ovb"), counts=False)

    fe = FE.FindErrors(FE.FeParameters(error_rate=a.erate))
    t0 = time.perf_counter()
    fe.load_reads(rs)
    load_s = time.perf_counter() - t0
    for _ in range(a.warmup):
        fe.run(store, bgn, end)
    times, stats = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        out = fe.run(store, bgn, end)
        times.append(time.perf_counter() - t0)
        stats.append(fe.stats())
    counters = fe.counters()
    if a.dump_dir:
        fe.write_red(os.path.join(a.dump_dir, "gpu.red"))
    k = int(np.argmin(times))
    best, st = times[k], stats[k]

    # parity: a few reads' overlaps alone give those reads' records (votes go to the A read)
    pick = [int(v) for v in np.linspace(bgn, end, a.parity_reads).astype(np.int64)]
    ok = True
    o = FR.defaults()
    o["erate"] = a.erate
    n_par = 0
    for rid in pick:
        sel = store[store["a"] == rid]
        n_par += int(sel.shape[0])
        reads = {rid: rs.read(rid - rs.first_iid)}
        for b in sel["b"]:
            reads[int(b)] = rs.read(int(b) - rs.first_iid)
        want, _, _ = FR.find_errors(sel, reads, rid, rid, o)
        ok &= bool(np.array_equal(out[out["readID"] == rid], want))
    fe.close()

    ms = st["ms_align"]
    line = {"bench": "findErrors", "reads": a.reads, "read_len": a.read_len,
            "read_error": a.read_error, "erate": a.erate, "overlaps": int(store.shape[0]),
            "records": int(out.shape[0]), "corrections": int(out.shape[0]) - rs.nreads,
            "find_errors_s": best, "find_errors_s_all": times,
            "overlaps_per_s": store.shape[0] / best,
            "aligned_bases": st["bases"], "g_aligned_bases_per_s": st["bases"] / best / 1e9,
            "rows": st["rows"], "m_rows_per_s": st["rows"] / best / 1e6,
            "kernel_ms": {"k_fe_align": ms, "k_fe_decide": st["ms_decide"]},
            "kernel_overlaps_per_s": store.shape[0] / (ms * 1e-3) if ms else None,
            "generic_alignments": st["n_generic"], "staged_alignments": st["n_staged"],
            "regrows": st["regrows"],
            "scratch_bytes": st["scratch_bytes"], "load_s": load_s, "overlapper_s": oic_s,
            "counters": counters,
            "parity": {"reads": pick, "overlaps": n_par, "of": int(store.shape[0]), "ok": ok}}
    print(json.dumps(line), flush=True)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
