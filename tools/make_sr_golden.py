#!/usr/bin/env python3
"""Write tests/golden/sr_*.npz from the reference splitReads.

    tools/make_sr_golden.py [--build-dir DIR] [--out tests/golden] [--only a,c]
    tools/make_sr_golden.py --time [--reads N]

The reference is compiled out of tree, into --build-dir (a temporary directory by default):
splitReads.C, splitReads-workUnit.C, splitReads-subReads.C, splitReads-trimBad.C, adjustNormal.C
and adjustFlipped.C with the oracle Makefile's REF_CXXFLAGS, linked under --gc-sections with the
objects `make -C oracle` leaves in oracle/_ref/obj.  Nothing of it is committed.

Each job is run as canu runs it (OverlapBasedTrimming.pm:128-196): the gkpStore by the reference's
gkStore code, with the three switches of each library (removeSpurReads, removeChimericReads,
checkForSubReads: bytes 152, 156 and 160 of a 168-byte record) set in its `libraries` file; the
overlap store by the reference's ovStore writer; the -Ci file written here; then
splitReads -G -O -Ci -Co -e -minlength -o [-t].  A fixture holds the read lengths, each read's
library flags, the store's records in store order, the input clear ranges, the options, and the
bytes of .clear, .log, .stats and stderr.  Fixture d also holds the two stores' files for the
executable test.

  a   the hand-made cases of `cases()`, -minlength 64
  b   the same, -minlength 0 and another -e
  c   the same, -t 5-40
  d   tests/golden/tr_d.npz's stores and the .clear the reference trimReads wrote for them,
      -t 3-99999 (clamped)

--time runs the reference on bench_sr.py's workload and prints its wall time.
"""
from __future__ import annotations

import argparse
import os
import struct
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

import sr_restate as SR  # noqa: E402
from make_co_golden import MHC_SRCS, REF, ref_cxxflags  # noqa: E402
from make_tr_golden import read_set  # noqa: E402

SR_SRCS = ["splitReads.C", "splitReads-workUnit.C", "splitReads-subReads.C", "splitReads-trimBad.C",
           "adjustNormal.C", "adjustFlipped.C"]
LIBRARY_BYTES, SPUR_AT, CHIMERA_AT, SUBREADS_AT = 168, 152, 156, 160
U32 = 0xFFFFFFFF


def build_reference(build_dir: str) -> str:
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    src = os.path.join(REF, "src", "overlapBasedTrimming")
    cxx = os.environ.get("CXX", "g++")
    procs, objs = [], []
    for s in SR_SRCS:
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
    out = os.path.join(build_dir, "sr_ref")
    subprocess.run([cxx, "-fopenmp", "-pthread", "-Wl,--gc-sections", "-o", out, *objs, "-lm"],
                   check=True)
    return out


def set_switches(gkp: str, lib_switches) -> None:
    """lib_switches: (spur, chimera, subreads) of library 1, 2, ..."""
    lp = os.path.join(gkp, "libraries")
    raw = bytearray(open(lp, "rb").read())
    assert len(raw) >= LIBRARY_BYTES * (len(lib_switches) + 1), len(raw)
    for k, sw in enumerate(lib_switches):
        for at, v in zip((SPUR_AT, CHIMERA_AT, SUBREADS_AT), sw):
            raw[LIBRARY_BYTES * (k + 1) + at:LIBRARY_BYTES * (k + 1) + at + 4] = struct.pack("<I", int(v))
    with open(lp, "wb") as f:
        f.write(raw)


def lib_flag(sw) -> int:
    return (SR.LIB_ELIGIBLE if any(sw) else 0) | (SR.LIB_SUBREADS if sw[2] else 0)


def clear_file(n, clear_in, entry0=(0, 0)) -> bytes:
    return struct.pack("<I", n) + struct.pack("<I", entry0[0]) + np.asarray(clear_in[0], "<u4").tobytes() + \
        struct.pack("<I", entry0[1]) + np.asarray(clear_in[1], "<u4").tobytes()


def splitreads_run(binary, d, gkp, store, clear_bytes_in, args):
    pre = os.path.join(d, "out")
    with open(pre + ".in.clear", "wb") as f:
        f.write(clear_bytes_in)
    t0 = time.time()
    cp = subprocess.run([binary, "-G", gkp, "-O", store, "-Ci", pre + ".in.clear", "-Co", pre + ".clear",
                         *args, "-o", pre], capture_output=True, cwd=d)
    dt = time.time() - t0
    if cp.returncode != 0:
        raise RuntimeError(f"splitReads failed ({cp.returncode}): {cp.stderr[-3000:]!r}")
    out = {"args": np.frombuffer(" ".join(args).encode(), dtype=np.uint8),
           "stderr": np.frombuffer(cp.stderr, dtype=np.uint8), "seconds": np.float64(dt)}
    for ext in ("clear", "log", "stats"):
        out[ext] = np.frombuffer(open(f"{pre}.{ext}", "rb").read(), dtype=np.uint8)
    return out


def store_files(out, gkp, store):
    for tag, path in (("gkp", gkp), ("ovs", store)):
        names = sorted(f for f in os.listdir(path) if os.path.isfile(os.path.join(path, f)))
        out[tag + "_names"] = np.array(names)
        for f in names:
            out[f"{tag}_file_{f}"] = np.frombuffer(open(os.path.join(path, f), "rb").read(), dtype=np.uint8)


def run_reference(binary, lengths, recs, libs, lib_switches, clear_in, args, keep_stores=False):
    """libs: the library (1-based) of every read.  -> dict of the fixture's arrays."""
    import oracle
    from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
    from canu_amd.synth import write_reads_file
    rs = read_set(lengths)
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
        set_switches(gkp, lib_switches)
        ovb = os.path.join(d, "in.ovb")
        write_ovb(np.array(recs, dtype=RECORD_DTYPE), ovb, counts=False)
        store = os.path.join(d, "asm.ovlStore")
        oracle.build_store(gkp, store, [ovb])
        stored = oracle.dump_store(gkp, store)
        out = splitreads_run(binary, d, gkp, store, clear_file(n, clear_in), args)
        out.update({"lengths": np.asarray(lengths, dtype=np.uint32),
                    "lib_flags": np.array([lib_flag(lib_switches[l - 1]) for l in libs], dtype=np.uint8),
                    "records": stored,
                    "clear_in": np.stack([np.asarray(clear_in[0], np.uint32), np.asarray(clear_in[1], np.uint32)])})
        if keep_stores:
            store_files(out, gkp, store)
    return out


# ------------------------------------------------------------------ the hand-made cases

LEN = 6000
BLO, BHI = 1000, 1400                                   # where a twin pair lies on its B read


class Builder:
    """Reads 1 .. are the cases' A reads, then the partners; a fresh partner per overlap pair."""

    def __init__(self):
        self.reads = []                                 # (length, library, clear)
        self.pending = []                               # (a, kind, args...)
        self.names = {}

    def read(self, name, length=LEN, lib=1, clear=None):
        self.reads.append((length, lib, clear))
        self.names[name] = len(self.reads)
        return len(self.reads)

    def single(self, a, abgn, aend, bbgn=BLO, bend=None, flipped=False, b=None):
        self.pending.append((a, b, [(abgn, aend, bbgn, bend if bend is not None else bbgn + (aend - abgn), flipped)]))

    def pair(self, a, first, second, b=None, same=False):
        """first / second: (abgn, aend[, bbgn, bend]); the first forward, the second flipped."""
        ovl = []
        for k, o in enumerate((first, second)):
            bb, be = (o[2], o[3]) if len(o) > 2 else (BLO, BHI)
            ovl.append((o[0], o[1], bb, be, bool(k) and not same))
        self.pending.append((a, b, ovl))

    def twins(self, a, junction, gap, count=1, span=400):
        for _ in range(count):
            self.pair(a, (junction - span, junction), (junction + gap, junction + gap + span))

    def finish(self, partner_lib=1):
        recs = []
        for a, b, ovl in self.pending:
            if b is None:
                self.reads.append((LEN, partner_lib, None))
                b = len(self.reads)
            for abgn, aend, bbgn, bend, fl in ovl:
                recs.append(SR.make_record(a, b, abgn, aend, self.reads[a - 1][0], bbgn, bend,
                                           self.reads[b - 1][0], fl))
        lens = [r[0] for r in self.reads]
        libs = [r[1] for r in self.reads]
        cb = [r[2][0] if r[2] else 0 for r in self.reads]
        ce = [r[2][1] if r[2] else r[0] for r in self.reads]
        return lens, recs, libs, (cb, ce)


LIB_SWITCHES = [(0, 0, 1), (1, 0, 0), (0, 0, 0), (1, 1, 1)]    # libraries 1 .. 4


def cases():
    B = Builder()
    a = B.read("three_small");      [B.twins(a, 3000, g) for g in (10, 20, 30)]
    a = B.read("two_small_weak");   B.twins(a, 3000, 10, 2)
    a = B.read("allhits_only");     B.twins(a, 3000, 10, 2); [B.pair(a, (2500, 2900), (3600, 4000)) for _ in range(4)]
    a = B.read("palindrome_only");  B.twins(a, 3000, 10, 2); B.pair(a, (500, 2000, 1000, 2500), (600, 2100, 1000, 2500))
    a = B.read("palindrome_1000");  B.twins(a, 3000, 10, 2); B.pair(a, (500, 2000, 1000, 2001), (1000, 2500, 1000, 2001))
    a = B.read("palindrome_1001");  B.twins(a, 3000, 10, 2); B.pair(a, (500, 2000, 1000, 2001), (999, 2500, 1000, 2001))
    a = B.read("span_ten");         B.twins(a, 3000, 10, 3); [B.single(a, 1000, 5000) for _ in range(10)]
    # nine span it, the tightest by one base at each end; two more miss by the margin exactly
    a = B.read("span_nine");        B.twins(a, 3000, 10, 3); [B.single(a, 1000, 5000) for _ in range(8)]
    B.single(a, 2899, 3111); B.single(a, 2900, 5000); B.single(a, 1000, 3110)
    a = B.read("gap_500");          B.twins(a, 3000, 500, 3)
    a = B.read("gap_501");          B.twins(a, 3000, 501, 3)
    a = B.read("ext_2000");         B.twins(a, 3000, 10, 2); [B.pair(a, (2100, 2500), (4500, 4900)) for _ in range(4)]
    a = B.read("ext_2001");         B.twins(a, 3000, 10, 2); [B.pair(a, (2100, 2500), (4501, 4901)) for _ in range(4)]
    a = B.read("a_ov_250");         [B.pair(a, (2000, 2650), (2400, 3000)) for _ in range(3)]
    a = B.read("a_ov_251");         [B.pair(a, (2000, 2651), (2400, 3000)) for _ in range(3)]
    a = B.read("b_ov_250");         [B.pair(a, (2600, 3000, 1000, 1400), (3010, 3400, 1150, 1550)) for _ in range(3)]
    a = B.read("b_ov_249");         [B.pair(a, (2600, 3000, 1000, 1400), (3010, 3400, 1151, 1551)) for _ in range(3)]
    a = B.read("disjoint");         [B.pair(a, (2600, 3000, 1000, 1400), (3010, 3400, 2000, 2400)) for _ in range(3)]
    a = B.read("zero_length");      B.twins(a, 3000, 0, 3)
    a = B.read("equal_pieces");     B.twins(a, 2900, 200, 3)
    a = B.read("middle_largest");   B.twins(a, 1000, 10, 3); B.twins(a, 5000, 10, 3)
    a = B.read("touching");         B.twins(a, 3000, 10, 2); B.twins(a, 3010, 10, 2)
    a = B.read("apart");            B.twins(a, 3000, 10, 3); B.twins(a, 3011, 10, 3)
    a = B.read("whole_bad", 400);   [B.pair(a, (0, 200), (0, 400)) for _ in range(3)]
    a = B.read("tie_jj");           [B.pair(a, (2000, 2200), (2000, 2500)) for _ in range(3)]
    a = B.read("short_pieces", 130);  [B.pair(a, (0, 60, 1000, 1400), (70, 130, 1000, 1400)) for _ in range(3)]
    # the snaps: the forward overlap ends 5 short of its B read's clear end, the flipped one
    # begins 5 into it; the A side has the room
    a = B.read("snap_full")
    [B.pair(a, (1600, 1995, 1000, LEN - 5), (2010, 2400, 5, 5000)) for _ in range(3)]
    a = B.read("snap_limited");     B.single(a, 4, 400, 10, 406); B.single(a, 5000, LEN - 4, 5000, LEN - 10)
    # half a base: a cut of 1 in 1024 on A is 0.5 of 512 on B, which round() takes up to 1;
    # the B sides then share 249 bases, not 250, and the snap back has no room on A
    a = B.read("half", clear=(1001, LEN))
    [B.pair(a, (1000, 2024, 0, 512), (2034, 3058, 0, 250)) for _ in range(3)]
    a = B.read("half_control", clear=(1001, LEN))
    [B.pair(a, (1000, 2024, 0, 512), (2034, 3058, 0, 251)) for _ in range(3)]
    a = B.read("miss_a", clear=(1000, 5000)); B.single(a, 0, 900); B.single(a, 5000, 5900); B.twins(a, 3000, 10, 3)
    a = B.read("no_coverage", clear=(1000, 5000)); B.single(a, 0, 1000)
    clipped = B.read("clipped_partner", clear=(2000, LEN))
    gone = B.read("deleted", clear=(U32, U32))
    a = B.read("miss_b");           B.single(a, 100, 1600, 0, 1500, b=clipped); B.twins(a, 3000, 10, 3)
    a = B.read("clipped_b");        B.single(a, 100, 3100, 1000, 4000, b=clipped)
    B.single(a, 200, 3200, 1000, 4000, True, b=clipped)
    a = B.read("deleted_b");        B.single(a, 100, 1600, b=gone); B.single(a, 200, 1700, b=gone)
    a = B.read("deleted_b_only");   B.single(a, 100, 1600, b=gone)
    a = B.read("group_three");      B.twins(a, 3000, 10, 3)
    a = B.read("same_orient");      B.pair(a, (2600, 3000), (3010, 3400), same=True); B.twins(a, 3000, 10, 3)
    a = B.read("no_overlaps")
    a = B.read("lib_spur_only", lib=2);  B.twins(a, 3000, 10, 3)
    a = B.read("lib_nothing", lib=3);    B.twins(a, 3000, 10, 3)
    a = B.read("lib_all", lib=4);        B.twins(a, 3000, 10, 3)
    spur_b = B.read("spur_partner", lib=2)
    a = B.read("palindrome_b_lib"); B.twins(a, 3000, 10, 2)
    B.pair(a, (500, 2000, 1000, 2500), (600, 2100, 1000, 2500), b=spur_b)
    # a group of three: two twin pairs' worth of overlaps with one partner
    g = B.names["group_three"]
    three = B.read("three_partner")
    B.pair(g, (2600, 3000), (3010, 3400), b=three)
    B.single(g, 3500, 3900, flipped=True, b=three)
    return B.finish()


def fixture(args):
    lens, recs, libs, clear_in = cases()
    return lens, recs, libs, LIB_SWITCHES, clear_in, args


def fixture_d(binary):
    """tr_d's two stores, the switches set, and the .clear the reference trimReads wrote."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "tr_d.npz"))
    n = int(fx["lengths"].shape[0])
    sw = [(0, 0, 1), (1, 1, 1)]
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        gkp, store = os.path.join(d, "ref.gkpStore"), os.path.join(d, "asm.ovlStore")
        for tag, path in (("gkp", gkp), ("ovs", store)):
            os.makedirs(path)
            for f in fx[tag + "_names"]:
                with open(os.path.join(path, str(f)), "wb") as F:
                    F.write(fx[f"{tag}_file_{f}"].tobytes())
        set_switches(gkp, sw)
        # which library each read is in: from the rule trimReads saw (library 1 has 1, 2 has 2)
        libs = [int(r) for r in fx["rules"]]
        clr = fx["clear"].tobytes()
        b, e = SR.parse_clear(clr, n)
        out = splitreads_run(binary, d, gkp, store, clr, ["-e", "0.015", "-minlength", "64", "-t", "3-99999"])
        out.update({"lengths": fx["lengths"], "records": fx["records"],
                    "lib_flags": np.array([lib_flag(sw[l - 1]) for l in libs], dtype=np.uint8),
                    "clear_in": np.stack([b[1:], e[1:]]), "clear_in_file": fx["clear"]})
        store_files(out, gkp, store)
    return out


FIXTURES = [("a", ["-e", "0.015", "-minlength", "64"]), ("b", ["-e", "0.3", "-minlength", "0"]),
            ("c", ["-e", "0.015", "-minlength", "64", "-t", "5-40"])]


def check(name: str, fx: dict) -> None:
    """The reference's output equals the restatement's, and the fixtures reach every branch."""
    P, rng = params_of(fx)
    R = SR.split_reads(fx["lengths"], fx["records"], fx["lib_flags"], tuple(fx["clear_in"]), P, rng)
    e0 = (0, 0)
    if "clear_in_file" in fx:
        b, e = SR.parse_clear(fx["clear_in_file"].tobytes())
        e0 = (int(b[0]), int(e[0]))
    for key, got in (("clear", SR.clear_bytes(R, e0)), ("log", SR.log_text(R).encode()),
                     ("stats", SR.stats_text(R, P).encode()),
                     ("stderr", SR.stderr_text(R, P, fx["records"]).encode())):
        if got != fx[key].tobytes():
            sys.stderr.write(f"--- reference {key}\n{fx[key].tobytes()[:3000]!r}\n--- restatement\n{got[:3000]!r}\n")
            raise AssertionError(f"fixture {name}: the restatement's {key} differs from the reference's")


def params_of(fx):
    from canu_amd.split_reads import parse_splitReads_args
    P, job = parse_splitReads_args(fx["args"].tobytes().decode().split() + "-G g -O o -Co c -o p".split())
    return SR.Params(P.erate, P.min_read_length), (job["id_min"], job["id_max"])


def time_reference(binary: str, n_reads: int) -> None:
    from canu_amd.split_reads import synth_store_view
    lengths, records, recs = synth_store_view(n_reads, with_input=True)
    t0 = time.time()
    fx = run_reference(binary, lengths, recs, [1] * len(lengths), [(0, 0, 1)],
                       (np.zeros(len(lengths), np.uint32), lengths), ["-e", "0.015", "-minlength", "64"])
    assert fx["records"].shape[0] == records.shape[0], (fx["records"].shape, records.shape)
    print(f"reference splitReads: {n_reads} reads, {fx['records'].shape[0]} overlaps in the store: "
          f"{float(fx['seconds']):.2f} s in splitReads ({time.time() - t0:.1f} s with the stores), "
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
    only = a.only.split(",") if a.only else None
    for name, args in FIXTURES + [("d", None)]:
        if only and name not in only:
            continue
        fx = fixture_d(binary) if name == "d" else run_reference(binary, *fixture(args))
        check(name, fx)
        fx.pop("seconds")
        path = os.path.join(a.out, f"sr_{name}.npz")
        np.savez_compressed(path, **fx)
        print(path, os.path.getsize(path), "bytes;", fx["lengths"].shape[0], "reads;",
              fx["records"].shape[0], "overlaps")
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
