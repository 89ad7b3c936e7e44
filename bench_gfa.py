#!/usr/bin/env python3
"""Measure the GPU alignGFA (canu_amd.align_gfa, libcanu_gfa.so) on one GPU.

    python bench_gfa.py [--links 512] [--records 64] [--steps 3]

The graph is synthetic (canu_amd.align_gfa.synth_graph): --links + 1 unitigs of --tig-len bases
with --overlap bases between neighbours at --error, every eighth link a false one; --records
unitigs of --utg-len bases placed on contigs of --ctg-len bases, every eighth 40 % off its
place.  One JSON line: links/s and records/s, DP cells/s (rows x columns of every pass: the
locate passes, the global pass, every split and every leaf), the ms of each kernel and of the
whole call, the counters, and a parity block: a sample of links and records against the Python
restatement of the reference (tests/gfa_restate.py).  tools/make_gfa_golden.py --time runs the
reference program on the same job.  No threshold is set here: the line is a measurement.
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
    ap.add_argument("--links", type=int, default=512)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--tig-len", type=int, default=12000)
    ap.add_argument("--overlap", type=int, default=2000)
    ap.add_argument("--utg-len", type=int, default=6000)
    ap.add_argument("--ctg-len", type=int, default=60000)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parity", type=int, default=4)
    return ap.parse_args(argv)


def main() -> None:
    a = parse_args()
    if a.gpus != 1:
        raise SystemExit("bench_gfa.py: alignGFA runs on one GPU")
    import numpy as np
    from canu_amd import align_gfa as G
    job = G.synth_graph(a.seed, a.links, a.records, a.tig_len, a.overlap, a.error, 8, a.ctg_len,
                        a.utg_len)
    import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py and the tests)
    import gfa_restate as GR

    g = G.AlignGFA()
    t0 = time.perf_counter()
    g.load_tigs(G.SET_T, job["utgs"])
    g.load_tigs(G.SET_C, job["ctgs"])
    load_s = time.perf_counter() - t0
    for _ in range(a.warmup):
        g.check_links(job["links"])
        g.check_records(job["records"])
    lt, ls, rt, rs = [], [], [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        lres, runs = g.check_links(job["links"])
        lt.append(time.perf_counter() - t0)
        ls.append(g.stats())
        t0 = time.perf_counter()
        rres, tries = g.check_records(job["records"])
        rt.append(time.perf_counter() - t0)
        rs.append(g.stats())
    g.close()
    kl, kr = int(np.argmin(lt)), int(np.argmin(rt))
    lbest, lst, rbest, rst = lt[kl], ls[kl], rt[kr], rs[kr]

    ok = True
    log = GR.new_log()
    picks_l = sorted({int(v) for v in np.linspace(0, a.links - 1, a.parity)}) if a.links else []
    for i in picks_l:
        l, r = job["links"][i], lres[i]
        link = {"Aid": int(l["a_id"]), "Afwd": bool(l["a_fwd"]), "Bid": int(l["b_id"]),
                "Bfwd": bool(l["b_fwd"]), "cigar": "%dM" % l["align"]}
        w = GR.check_link(link, job["utgs"], log, None)
        got = G.cigar_text(runs[int(r["run_off"]):int(r["run_off"]) + int(r["n_runs"])])
        ok &= (got if r["success"] else None) == w["cigar"] and int(r["abgn"]) == w["abgn"] and \
            int(r["bend"]) == w["bend"]
    picks_r = sorted({int(v) for v in np.linspace(0, a.records - 1, a.parity)}) if a.records else []
    for i in picks_r:
        q, r = job["records"][i], rres[i]
        rec = {"Aid": int(q["a_id"]), "Bid": int(q["b_id"]), "Bfwd": bool(q["b_fwd"]),
               "bgn": int(q["bgn"]), "end": int(q["end"]), "Aname": "c", "Bname": "u", "score": 0}
        wok, wt = GR.check_record(rec, job["ctgs"], job["utgs"], log, None)
        ok &= bool(r["success"]) == wok and (int(r["bgn"]), int(r["end"])) == (rec["bgn"], rec["end"]) \
            and int(r["n_tries"]) == len(wt)

    link_ms = {n: lst["ms_" + n] for n in ("extend_b", "extend_a", "final")}
    lk_ms = sum(link_ms.values())
    line = {"bench": "alignGFA", "links": a.links, "records": a.records, "tig_len": a.tig_len,
            "overlap": a.overlap, "utg_len": a.utg_len, "ctg_len": a.ctg_len, "error": a.error,
            "links_s": lbest, "links_s_all": lt, "links_per_s": a.links / lbest if lbest else None,
            "links_kept": int(lres["success"].sum()), "cigar_runs": int(runs.shape[0]),
            "link_dp_cells": lst["dp_cells"], "link_t_cells_per_s": lst["dp_cells"] / lbest / 1e12,
            "link_kernel_ms": link_ms,
            "link_kernel_t_cells_per_s": lst["dp_cells"] / (lk_ms * 1e-3) / 1e12 if lk_ms else None,
            "leaves": lst["n_leaves"], "splits": lst["n_splits"], "link_batches": lst["n_batches"],
            "link_scratch_bytes": lst["scratch_bytes"],
            "records_s": rbest, "records_s_all": rt,
            "records_per_s": a.records / rbest if rbest else None,
            "records_kept": int(rres["success"].sum()), "tries": int(tries.shape[0]),
            "record_rounds": rst["n_rounds"], "record_dp_cells": rst["dp_cells"],
            "record_t_cells_per_s": rst["dp_cells"] / rbest / 1e12,
            "record_kernel_ms": rst["ms_records"],
            "record_kernel_t_cells_per_s": rst["dp_cells"] / (rst["ms_records"] * 1e-3) / 1e12
            if rst["ms_records"] else None,
            "load_s": load_s,
            "parity": {"links": picks_l, "records": picks_r, "ok": bool(ok)}}
    print(json.dumps(line), flush=True)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
