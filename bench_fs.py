#!/usr/bin/env python3
"""Measure the GPU falconsense (canu_amd.falconsense, libcanu_fs.so) on one GPU.

    python bench_fs.py [--templates 512] [--read-len 4000] [--coverage 12] [--steps 3]

The layouts are synthetic (canu_amd.falconsense.synth_layouts): reads of about --read-len at
--coverage and --read-error from one genome, each read the template of the reads that overlap it
by 1,000 bases or more, placed where the genome puts them.  One JSON line: templates/s, evidence
alignments/s, DP cells/s (rows x columns of every pass: the two locate passes, every split and
every leaf), the ms of each kernel, the counters, and a parity block: the consensus of a few
templates against the Python restatement of the reference (tests/fs_restate.py).
tools/make_fs_golden.py --time runs the reference program on the same layouts.  No threshold is
set here: the line is a measurement.
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


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--templates", type=int, default=512)
    ap.add_argument("--read-len", type=int, default=4000)
    ap.add_argument("--coverage", type=int, default=12)
    ap.add_argument("--read-error", type=float, default=0.10)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--parity-templates", type=int, default=3)
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_fs.py: falconsense runs on one GPU")
    import numpy as np
    from canu_amd.falconsense import FalconSense, FsParameters, synth_layouts
    from canu_amd.synth import ReadSet
    reads, layouts, children = synth_layouts(a.templates, a.read_len, a.coverage, a.read_error, a.seed)
    import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py and the tests)
    import fs_restate as FS

    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    rs = ReadSet(bases=np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets=offs,
                 lengths=lens, first_iid=1)
    P = FsParameters()                                    # canu's: -cc 4 -cl 500, -ci 0 by atoi
    fs = FalconSense(P)
    t0 = time.perf_counter()
    fs.load_reads(rs)
    load_s = time.perf_counter() - t0
    for _ in range(a.warmup):
        fs.run(layouts, children)
    times, stats = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        cns = fs.run(layouts, children)
        times.append(time.perf_counter() - t0)
        stats.append(fs.stats())
    fasta = fs.fasta_bytes()
    fs.close()
    k = int(np.argmin(times))
    best, st = times[k], stats[k]

    pick = sorted({int(v) for v in np.linspace(0, a.templates - 1, a.parity_templates)})
    rd = {i + 1: r for i, r in enumerate(reads)}
    ok = True
    for t in pick:
        l = layouts[t]
        ch = [tuple(int(v) for v in c) for c in
              children[int(l["first_child"]):int(l["first_child"]) + int(l["n_children"])]]
        want, _ = FS.correct_tig(rd, int(l["tig_id"]), ch, P.min_coverage, P.min_identity)
        ok &= cns[t] == want

    kernels = {n: st["ms_" + n] for n in ("locate", "path", "sort", "consensus")}
    align_ms = kernels["locate"] + kernels["path"]
    line = {"bench": "falconsense", "templates": a.templates, "read_len": a.read_len,
            "coverage": a.coverage, "read_error": a.read_error,
            "children": int(layouts["n_children"].sum()), "template_bases": int(lens.sum()),
            "falconsense_s": best, "falconsense_s_all": times,
            "templates_per_s": a.templates / best,
            "evidence_alignments": st["n_aligned"] + st["n_rejected"],
            "evidence_alignments_per_s": (st["n_aligned"] + st["n_rejected"]) / best,
            "dp_cells": st["dp_cells"], "t_cells_per_s": st["dp_cells"] / best / 1e12,
            "kernel_ms": kernels,
            "kernel_t_cells_per_s": st["dp_cells"] / (align_ms * 1e-3) / 1e12 if align_ms else None,
            "tags": st["n_tags"], "leaves": st["n_leaves"], "splits": st["n_splits"],
            "aligned": st["n_aligned"], "skipped": st["n_skipped"], "rejected": st["n_rejected"],
            "batches": st["n_batches"], "scratch_bytes": st["scratch_bytes"], "load_s": load_s,
            "corrected_reads": fasta.count(b">"), "corrected_bases": len(fasta) - fasta.count(b"\n")
            - sum(len(h) for h in fasta.split(b"\n") if h.startswith(b">")),
            "parity": {"templates": [int(layouts[t]["tig_id"]) for t in pick], "ok": bool(ok)}}
    print(json.dumps(line), flush=True)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
