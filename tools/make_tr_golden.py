#!/usr/bin/env python3
"""Write tests/golden/tr_*.npz from the reference trimReads.

    tools/make_tr_golden.py [--build-dir DIR] [--out tests/golden] [--only a,b1]
    tools/make_tr_golden.py --time [--reads N]

The reference is compiled out of tree, into --build-dir (a temporary directory by default):
trimReads.C, trimReads-largestCovered.C and trimReads-bestEdge.C with the oracle Makefile's
REF_CXXFLAGS, linked under --gc-sections with the objects `make -C oracle` leaves in
oracle/_ref/obj (fe_configure.o for AS_configure, the stores, decodeRange).  Nothing of it is
committed.

Each job is run as canu runs it (OverlapBasedTrimming.pm:57-120): the gkpStore by the reference's
gkStore code, with `_finalTrim` of each library set in its `libraries` file (byte 144 of a
168-byte record); the overlap store by the reference's ovStore writer; then
trimReads -G -O -Co -e -minlength -ol -oc -o [-t].  A fixture holds the read lengths, each read's
rule, the store's records in store order, the options, and the bytes of .clear, .log, .stats and
stderr.  The reference's .dat / .gp plot files are not kept.  Fixture d also holds the two stores'
files for the executable test; its reads are all A, trimReads never looks at a base.

  a   reads cut from a genome, chimeric and thinly covered ends among them, overlapped by the
      CPU oracle of overlapInCore: MOD, NOC, DEL and NOV all occur
  b0..b3  the hand-made cases of CASES_B plus random intervals on a coarse grid, -oc 0 / 1 / 2 / 3
  c   rule 2 (bestEdge) on every read
  d   two libraries, rules 1 and 2, -t 5-30

--time runs the reference on bench_tr.py's workload and prints its wall time.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tr_restate as TR  # noqa: E402
from make_co_golden import MHC_SRCS, REF, ref_cxxflags  # noqa: E402

TR_SRCS = ["trimReads.C", "trimReads-largestCovered.C", "trimReads-bestEdge.C"]
UTG_ONLY = 4                                           # forUTG: the store keeps the overlap
LIBRARY_BYTES, FINALTRIM_AT = 168, 144


def build_reference(build_dir: str) -> str:
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    src = os.path.join(REF, "src", "overlapBasedTrimming")
    cxx = os.environ.get("CXX", "g++")
    procs, objs = [], []
    for s in TR_SRCS:
        o = os.path.join(build_dir, s + ".o")
        procs.append(subprocess.Popen([cxx, *ref_cxxflags(), "-I" + src, "-c", os.path.join(src, s),
                                       "-o", o]))
        objs.append(o)
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("the reference did not compile")
    objs.append(os.path.join(obj, "fe_configure.o"))
    objs += [os.path.join(obj, s.replace("/", "__") + ".o") for s in MHC_SRCS]
    objs += [os.path.join(obj, "AS_UTL__AS_UTL_decodeRange.C.o"),
             os.path.join(obj, "AS_UTL__timeAndSize.C.o")]
    for o in objs:
        if not os.path.exists(o):
            raise FileNotFoundError(f"{o}: run `make -C oracle` first")
    out = os.path.join(build_dir, "tr_ref")
    subprocess.run([cxx, "-fopenmp", "-pthread", "-Wl,--gc-sections", "-o", out, *objs, "-lm"],
                   check=True)
    return out


def read_set(lengths, reads=None):
    from canu_amd.synth import ReadSet
    lens = np.asarray(lengths, dtype=np.uint32)
    offs = np.zeros(lens.shape[0], dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if reads is not None else \
        np.full(int(lens.sum()), ord("A"), dtype=np.uint8)
    return ReadSet(bases=bases, offsets=offs, lengths=lens, first_iid=1)


def run_reference(binary, lengths, recs, libs, lib_rules, args, keep_stores=False, reads=None):
    """libs: the library (1-based) of every read; lib_rules: finalTrim of library 1, 2, ...
    -> dict of the fixture's arrays."""
    import oracle
    from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
    from canu_amd.synth import write_reads_file
    rs = read_set(lengths, reads)
    n = len(lengths)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        rf = os.path.join(d, "reads.bin")
        write_reads_file(rf, rs)
        lf = os.path.join(d, "libs.bin")
        np.asarray(libs, dtype=np.uint32).tofile(lf)
        cp = subprocess.run([oracle.REF_BIN, rf, os.path.join(d, "w"), "-", "--gkp-only", "--libs", lf],
                            capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"oic_ref --gkp-only failed: {cp.stderr[-2000:]}")
        gkp = os.path.join(d, "w", "ref.gkpStore")
        lp = os.path.join(gkp, "libraries")
        raw = bytearray(open(lp, "rb").read())
        assert len(raw) >= LIBRARY_BYTES * (len(lib_rules) + 1), len(raw)
        for k, rule in enumerate(lib_rules):
            at = LIBRARY_BYTES * (k + 1) + FINALTRIM_AT
            assert raw[at:at + 4] == b"\x01\0\0\0", "not where _finalTrim lies"
            raw[at] = rule
        with open(lp, "wb") as f:
            f.write(raw)
        ovb = os.path.join(d, "in.ovb")
        write_ovb(np.array(recs, dtype=RECORD_DTYPE), ovb, counts=False)
        store = os.path.join(d, "asm.ovlStore")
        oracle.build_store(gkp, store, [ovb])
        stored = oracle.dump_store(gkp, store)
        pre = os.path.join(d, "out")
        t0 = time.time()
        cp = subprocess.run([binary, "-G", gkp, "-O", store, "-Co", pre + ".clear", *args, "-o", pre],
                            capture_output=True, cwd=d)
        dt = time.time() - t0
        if cp.returncode != 0:
            raise RuntimeError(f"trimReads failed ({cp.returncode}): {cp.stderr[-3000:]!r}")
        out = {"lengths": np.asarray(lengths, dtype=np.uint32),
               "rules": np.array([lib_rules[l - 1] for l in libs], dtype=np.uint8),
               "records": stored,
               "args": np.frombuffer(" ".join(args).encode(), dtype=np.uint8),
               "stderr": np.frombuffer(cp.stderr, dtype=np.uint8), "seconds": np.float64(dt)}
        for ext in ("clear", "log", "stats"):
            out[ext] = np.frombuffer(open(f"{pre}.{ext}", "rb").read(), dtype=np.uint8)
        if keep_stores:
            for tag, path in (("gkp", gkp), ("ovs", store)):
                names = sorted(f for f in os.listdir(path) if os.path.isfile(os.path.join(path, f)))
                out[tag + "_names"] = np.array(names)
                for f in names:
                    out[f"{tag}_file_{f}"] = np.frombuffer(open(os.path.join(path, f), "rb").read(),
                                                           dtype=np.uint8)
    return out


# ------------------------------------------------------------------ the hand-made cases

CANU_ARGS = ["-e", "0.015", "-minlength", "64", "-ol", "40"]
BAD_EV, CASES_B, CASES_C = TR.BAD_EV, TR.CASES_B, TR.CASES_C


def hand_records(cases, first_partner, rng=None):
    """Read k + 1 carries cases[k]; the partner of every overlap is one of the reads from
    first_partner on, whose twin overlap covers the whole partner."""
    lens, recs = [], []
    for k, (_, ivs) in enumerate(cases):
        lens.append(1000)
        for j, iv in enumerate(ivs):
            ev = iv[2] if len(iv) > 2 else 0
            recs.append(TR.make_record(k + 1, first_partner + (j % 4), iv[0], iv[1], 1000, ev, UTG_ONLY))
    return lens, recs


def random_cases(seed, n, grid=50, length=1000):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(2, 9))
        ivs = []
        for _ in range(m):
            lo = int(rng.integers(0, length // grid)) * grid
            hi = min(length, lo + int(rng.integers(1, 9)) * grid)
            if lo < hi:
                ivs.append((lo, hi, BAD_EV if rng.random() < 0.15 else 0))
        if rng.random() < 0.4 and ivs:
            ivs.append(ivs[0])
        out.append((f"random{k}", ivs or [(0, 100)]))
    return out


def fixture_b(oc):
    cases = CASES_B + random_cases(7301, 30)
    n = len(cases)
    lens, recs = hand_records(cases, n + 2)
    lens += [1000] * 5                                  # one read without overlaps, four partners
    return lens, recs, [1] * len(lens), [1], CANU_ARGS + ["-oc", str(oc)]


def fixture_c():
    cases = CASES_C + random_cases(7302, 40, grid=20)
    n = len(cases)
    lens, recs = hand_records(cases, n + 2)
    lens += [1000] * 5
    return lens, recs, [1] * len(lens), [2], CANU_ARGS + ["-oc", "1"]


def fixture_d():
    cases = random_cases(7303, 36, grid=25, length=400)
    n = len(cases)
    lens, recs = [], []
    for k, (_, ivs) in enumerate(cases):
        lens.append(400)
        for j, iv in enumerate(ivs):
            recs.append(TR.make_record(k + 1, n + 2 + (j % 4), iv[0], iv[1], 400, iv[2], UTG_ONLY))
    lens += [400] * 5
    libs = [1 + (k % 3 == 0) for k in range(len(lens))]
    return lens, recs, libs, [1, 2], CANU_ARGS + ["-oc", "2", "-t", "5-30"]


def fixture_a():
    """Reads of a genome overlapped by the CPU oracle: honest reads, chimeras of two distant
    stretches, reads with a stretch of junk at an end and a read of junk only, at a coverage
    whose thin places -oc 2 cuts."""
    import oracle
    import make_fe_golden as MG
    S = MG.Sample(7300, 9000, 36, 0.01, lo=900, hi=1800)
    rng = S.rng
    for k in range(6):                                  # chimeras
        s1, s2 = int(rng.integers(0, 3000)), int(rng.integers(5000, 8000))
        a = MG._mutate(rng, S.genome[s1:s1 + 700], 0.01)[0]
        b = MG._mutate(rng, S.genome[s2:s2 + 700], 0.01)[0]
        S.add_raw(a + (MG._rc(b) if k & 1 else b))
    for k in range(5):                                  # junk ends
        s = int(rng.integers(0, 7500))
        body = MG._mutate(rng, S.genome[s:s + 1200], 0.01)[0]
        S.add_raw(MG._rand(rng, 150 + 40 * k) + body if k & 1 else body + MG._rand(rng, 150 + 40 * k))
    S.add_raw(MG._rand(rng, 1000))                      # junk only: no overlaps
    rs = MG.read_set(S.reads)
    P = oracle.default_params(Kmer_Len=22, maxErate=float(np.float32(0.06)), Min_Olap_Len=100,
                              Doing_Partial_Overlaps=True)
    got = oracle.run_oracle(rs, P)
    recs = [tuple(int(v) for v in r) for r in got]
    lens = [len(r) for r in S.reads]
    return lens, recs, [1] * len(lens), [1], ["-e", "0.03", "-minlength", "1000", "-ol", "40", "-oc", "2"], S.reads


FIXTURES = [("a", fixture_a), ("b0", lambda: fixture_b(0)), ("b1", lambda: fixture_b(1)),
            ("b2", lambda: fixture_b(2)), ("b3", lambda: fixture_b(3)), ("c", fixture_c),
            ("d", fixture_d)]


def check(name: str, fx: dict) -> None:
    """Each fixture reaches what it is for, on the reference's own output."""
    log = fx["log"].tobytes().decode().splitlines()[1:]
    rows = {int(l.split("\t")[0]): l.split("\t") for l in log}
    tags = {r[5] for r in rows.values()}
    if name == "a":
        assert tags == {"MOD", "NOC", "DEL", "NOV"}, tags
    if name.startswith("b"):
        oc = int(name[1])
        case = {c[0]: k + 1 for k, c in enumerate(CASES_B)}
        if oc < 2:                                      # one overlap deep
            assert rows[case["wrap"]][3:6] == (["0", "900", "MOD"] if oc == 0 else ["500", "900", "MOD"])
            assert rows[case["two_winners"]][3:5] == ["0", "300"]
            assert rows[case["minlength_m1"]][5] == "DEL" and rows[case["minlength"]][5] == "MOD"
        assert rows[case["all_skipped"]][5:] == ["DEL", "no high quality overlaps"]
        assert rows[case["full"]][5] == ("NOC" if oc < 2 else "DEL")
        if oc >= 2:
            assert rows[case["depth_hole"]][3:5] in (["0", "400"], ["600", "1000"]), rows[case["depth_hole"]]
        if oc == 2:                                     # computeDepth's rewritten count
            assert rows[case["depth_rewrite"]][5:] == ["DEL", "no high quality overlaps"]
    if name == "c":
        assert rows[1][3:5] == ["52", "998"], rows[1]
    if name == "d":
        assert min(rows) == 5 and max(rows) == 30


def time_reference(binary: str, n_reads: int) -> None:
    from canu_amd.trim_reads import synth_store_view
    lengths, records, recs = synth_store_view(n_reads, with_input=True)   # the store adds the twins
    t0 = time.time()
    fx = run_reference(binary, lengths, recs, [1] * len(lengths), [1], CANU_ARGS + ["-oc", "1"])
    assert fx["records"].shape[0] == records.shape[0]
    print(f"reference trimReads: {n_reads} reads, {fx['records'].shape[0]} overlaps in the store: "
          f"{float(fx['seconds']):.2f} s in trimReads ({time.time() - t0:.1f} s with the stores), "
          f"{n_reads / float(fx['seconds']):.0f} reads/s")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reads", type=int, default=200_000)
    a = ap.parse_args()
    tmp = None
    bd = a.build_dir
    if bd is None:
        tmp = tempfile.TemporaryDirectory()
        bd = tmp.name
    os.makedirs(bd, exist_ok=True)
    assert not os.path.abspath(bd).startswith(ROOT + os.sep), "build outside the repository"
    binary = build_reference(bd)
    if a.time:
        time_reference(binary, a.reads)
        return 0
    os.makedirs(a.out, exist_ok=True)
    for name, mk in FIXTURES:
        if a.only and name not in a.only.split(","):
            continue
        made = mk()
        lens, recs, libs, lib_rules, args = made[:5]
        fx = run_reference(binary, lens, recs, libs, lib_rules, args, keep_stores=(name == "d"),
                           reads=made[5] if len(made) > 5 else None)
        check(name, fx)
        fx.pop("seconds")
        path = os.path.join(a.out, f"tr_{name}.npz")
        np.savez_compressed(path, **fx)
        log = fx["log"].tobytes().decode()
        print(path, os.path.getsize(path), "bytes;", len(lens), "reads;", fx["records"].shape[0],
              "overlaps;", {t: log.count("\t" + t) for t in ("NOV", "DEL", "NOC", "MOD")})
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
