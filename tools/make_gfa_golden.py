#!/usr/bin/env python3
"""Write tests/golden/gfa_*.npz from the reference alignGFA.

    tools/make_gfa_golden.py [--build-dir DIR] [--out tests/golden] [--only a,b]
    tools/make_gfa_golden.py --time [--links N] [--records N] [--threads T]

The reference is compiled out of tree, into --build-dir (a temporary directory by default):
gfa/alignGFA.C, gfa.C, bed.C, stores/tgStore.C, tgTig.C, utgcns/stashContains.C and
overlapInCore/libedlib/edlib.C with the oracle Makefile's REF_CXXFLAGS, linked under
--gc-sections with the objects `make -C oracle` leaves in oracle/_ref/obj (gkStore,
gkStoreEncode, AS_UTL_fileIO, AS_UTL_reverseComplement, and fe_configure.o standing in for
AS_configure).  Nothing of it is committed.

The tig stores are encoded here (tests/gfa_restate.py: encode_tigstore -- record, bases,
quality values, svID 2, deleted entries); the reference reading them back is the check of the
encoder: the LN:i: values it prints are the ungapped lengths.  Each job runs with -t 1, plain
and with -V, in a directory of its own under relative names, so that stderr names no path.

  a  -gfa: links kept and dropped in all four orientations, circular links (one to the same
     end), extend B failing before extend A, both clamps, a query longer than its target,
     CIGARs with I and D, a gapped consensus, a deleted tig, N against N in both senses
  b  -bed -C: placements accepted at both contig ends, an edge moved out on either side,
     RELAX followed by success and by ABORT, a reversed unitig
  c  -bed -C: a unitig of 50,000 bases (LEFT / RIGHT, each the whole of it) and one of 49,999,
     reversed
  d  -bed without -C: kept and failed ('*') links, a pair on different contigs, a thin
     intersection
  e  -bed -C: a reversed unitig of 52,000 bases, LEFT and RIGHT apart

--time runs the reference on canu_amd.align_gfa.synth_graph's job and prints its wall time:
the figure DESIGN.md sets beside bench_gfa.py's.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gfa_restate as GR  # noqa: E402
from make_co_golden import REF, ref_cxxflags  # noqa: E402

SRCS = ["gfa/alignGFA.C", "gfa/gfa.C", "gfa/bed.C", "stores/tgStore.C", "stores/tgTig.C",
        "utgcns/stashContains.C", "overlapInCore/libedlib/edlib.C"]
SHARED = ["stores/gkStore.C", "stores/gkStoreEncode.C", "AS_UTL/AS_UTL_fileIO.C",
          "AS_UTL/AS_UTL_reverseComplement.C"]
EXTRA_INC = ["gfa", "overlapInCore/libedlib", "utgcns"]


def build_reference(build_dir: str) -> str:
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    cxx = os.environ.get("CXX", "g++")
    flags = ref_cxxflags() + ["-I" + os.path.join(REF, "src", d) for d in EXTRA_INC]
    procs, objs = [], []
    for s in SRCS:
        o = os.path.join(build_dir, s.replace("/", "__") + ".o")
        procs.append(subprocess.Popen([cxx, *flags, "-c", os.path.join(REF, "src", s), "-o", o]))
        objs.append(o)
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("the reference did not compile")
    shared = [os.path.join(obj, "fe_configure.o")]
    shared += [os.path.join(obj, s.replace("/", "__") + ".o") for s in SHARED]
    for o in shared:
        if not os.path.exists(o):
            raise FileNotFoundError(f"{o}: run `make -C oracle` first")
    out = os.path.join(build_dir, "gfa_ref")
    subprocess.run([cxx, "-fopenmp", "-pthread", "-Wl,--gc-sections", "-o", out, *objs, *shared,
                    "-lm"], check=True)
    return out


def write_store(path: str, gapped: list, version: int = 2) -> None:
    os.makedirs(path)
    tig, dat = GR.encode_tigstore(gapped, version)
    for ext, raw in (("tig", tig), ("dat", dat)):
        with open(os.path.join(path, "seqDB.v%03d.%s" % (version, ext)), "wb") as f:
            f.write(raw)


def run_reference(ref: str, args: list, T: list, C: list | None, text: str, verbose: bool,
                  threads: int = 1):
    """-> (output file, stderr, seconds).  args name T.tigStore, C.tigStore, in and out."""
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        write_store(os.path.join(d, "T.tigStore"), T)
        if C is not None:
            write_store(os.path.join(d, "C.tigStore"), C)
        with open(os.path.join(d, "in"), "w") as f:
            f.write(text)
        cmd = [ref, *args, "-t", str(threads)] + (["-V"] if verbose else [])
        t0 = time.time()
        cp = subprocess.run(cmd, capture_output=True, cwd=d)
        dt = time.time() - t0
        if cp.returncode != 0:
            raise RuntimeError(f"alignGFA failed ({cp.returncode}): {cp.stderr[-3000:]!r}")
        with open(os.path.join(d, "out")) as f:
            out = f.read()
    return out, cp.stderr.decode(), dt


# ------------------------------------------------------------------ the jobs

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rand_seq(rng, n: int) -> bytes:
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def mutate(rng, seq: bytes, rate: float) -> bytes:
    """Substitutions, insertions and deletions, a third each."""
    out = bytearray()
    for ch in seq:
        if rng.random() < rate:
            kind = int(rng.integers(0, 3))
            if kind == 0:
                out.append(int(_ACGT[(b"ACGT".index(ch) + int(rng.integers(1, 4))) % 4]))
            elif kind == 1:
                out.append(ch)
                out.append(int(_ACGT[int(rng.integers(0, 4))]))
            continue
        out.append(ch)
    return bytes(out)


def with_gaps(rng, seq: bytes, n: int) -> bytes:
    out = bytearray(seq)
    for p in sorted((int(x) for x in rng.integers(1, len(seq) - 1, n)), reverse=True):
        out[p:p] = b"-"
    return bytes(out)


def rc(seq: bytes) -> bytes:
    return seq.translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


def gfa_text(tigs: list, links: list) -> str:
    out = ["H\tVN:Z:bogart/edges\n"]
    for i, t in enumerate(tigs):
        if t is not None:                              # lengths that the program must reset
            out.append("S\ttig%08d\t*\tLN:i:%d\n" % (i, len(t) + 7))
    for (a, sa, b, sb, cigar) in links:
        out.append("L\ttig%08d\t%s\ttig%08d\t%s\t%s\n" % (a, sa, b, sb, cigar))
    return "".join(out)


def fixture_a():
    rng = np.random.default_rng(9101)
    g = rand_seq(rng, 11000)
    g2 = bytearray(rand_seq(rng, 6000))
    for p in (2100, 2300, 4200):
        g2[p] = ord("N")
    g2 = bytes(g2)
    c = rand_seq(rng, 2000)
    tigs = [
        g[0:3000],                                     # 0
        with_gaps(rng, mutate(rng, g[2500:5500], 0.03), 25),   # 1: a gapped consensus
        rc(mutate(rng, g[5000:8000], 0.02)),           # 2
        rc(g[7400:9500]),                              # 3
        mutate(rng, g[9000:11000], 0.01),              # 4
        c + c[:400],                                   # 5: its end repeats its begin
        g[2600:3000],                                  # 6: shorter than its overlap
        g[2500:3020],                                  # 7: shorter than 1.1 x its overlap
        None,                                          # 8: deleted, not referenced
        g2[0:2500],                                    # 9: N, forward
        rc(g2[2000:4500]),                             # 10: N, reversed
        rc(g2[4000:6000]),                             # 11
    ]
    links = [
        (0, "+", 1, "+", "500M"),
        (1, "+", 2, "-", "450M20I30M10D20M"),
        (2, "-", 3, "-", "600M"),
        (3, "-", 4, "+", "500M"),
        (0, "+", 4, "+", "400M"),                      # no overlap: dropped
        (5, "+", 5, "+", "400M"),                      # circular
        (5, "+", 5, "-", "400M"),                      # circular to the same end
        (0, "+", 1, "+", "300M300I"),                  # extend B fails, extend A succeeds
        (4, "+", 0, "+", "300M300D"),                  # nothing aligns; the query is longer
        (6, "+", 1, "+", "500M"),                      # Abgn clamped to 0
        (0, "+", 7, "+", "500M"),                      # Bend clamped to Blen
        (9, "+", 10, "-", "500M"),                     # N forward against N reversed
        (10, "-", 11, "-", "500M"),                    # N reversed against N reversed
        (4, "-", 3, "+", "500M"),                      # the fourth link again from the other side
    ]
    args = "-T T.tigStore 2 -gfa -i in -o out".split()
    return args, tigs, None, gfa_text(tigs, links)


def bed_text(recs: list) -> str:
    return "".join("ctg%08d\t%d\t%d\tutg%08d\t%d\t%s\n" % r for r in recs)


def fixture_b():
    rng = np.random.default_rng(9102)
    c0, c1 = rand_seq(rng, 6000), rand_seq(rng, 3000)
    utgs = [
        c0[2000:2800],                                 # 0: placed exactly: the left edge moves
        c0[0:700],                                     # 1: at the contig's begin
        c0[3600:4400],                                 # 2: placed 600 too far left: RELAX, right edge
        rand_seq(rng, 500),                            # 3: from nowhere: RELAX to ABORT
        rc(mutate(rng, c1[500:1500], 0.01)),           # 4: reversed
        c1[2400:3000],                                 # 5: at the contig's end
        None,
    ]
    recs = [(0, 2000, 2800, 0, 7, "+"), (0, 0, 700, 1, 0, "+"), (0, 3000, 3800, 2, 0, "+"),
            (0, 4000, 4500, 3, 0, "+"), (1, 480, 1510, 4, 0, "-"), (1, 2400, 3000, 5, 0, "+")]
    args = "-T T.tigStore 2 -C C.tigStore 2 -bed -i in -o out".split()
    return args, utgs, [c0, c1], bed_text(recs)


def fixture_c():
    rng = np.random.default_rng(9103)
    c0 = rand_seq(rng, 58000)
    utgs = [mutate(rng, c0[3000:53200], 0.004)[:50000], rc(c0[4000:53999])]
    recs = [(0, 3000, 53000, 0, 0, "+"), (0, 4100, 54099, 1, 0, "-")]
    args = "-T T.tigStore 2 -C C.tigStore 2 -bed -i in -o out".split()
    return args, utgs, [c0], bed_text(recs)


def fixture_e():
    rng = np.random.default_rng(9105)
    c0 = rand_seq(rng, 56000)
    utgs = [rc(mutate(rng, c0[2500:54600], 0.004)[:52000])]
    recs = [(0, 2400, 54400, 0, 0, "-")]
    args = "-T T.tigStore 2 -C C.tigStore 2 -bed -i in -o out".split()
    return args, utgs, [c0], bed_text(recs)


def fixture_d():
    rng = np.random.default_rng(9104)
    g = rand_seq(rng, 8000)
    utgs = [g[0:3000], g[2500:5500], g[5450:8000], rand_seq(rng, 2000), rand_seq(rng, 2000),
            mutate(rng, g[100:3100], 0.02), None]
    recs = [(0, 0, 3000, 0, 0, "+"), (0, 2500, 5500, 1, 0, "-"), (0, 5450, 8000, 2, 0, "+"),
            (1, 0, 2000, 3, 0, "+"), (0, 1000, 3000, 4, 0, "+"), (0, 100, 3100, 5, 0, "+")]
    args = "-T T.tigStore 2 -bed -i in -o out".split()
    return args, utgs, None, bed_text(recs)


FIXTURES = [("a", fixture_a), ("b", fixture_b), ("c", fixture_c), ("d", fixture_d),
            ("e", fixture_e)]


def tig_arrays(prefix: str, tigs: list) -> dict:
    """Deleted, all-ACGT (2 bits a base) and other tigs, as tests/gfa_restate.py reads them."""
    lens, kinds, packed, raw = [], [], [], bytearray()
    for t in tigs:
        if t is None:
            lens.append(0)
            kinds.append(0)
        elif set(t) <= set(b"ACGT"):
            lens.append(len(t))
            kinds.append(1)
            packed.append(GR.pack2(t))
        else:
            lens.append(len(t))
            kinds.append(2)
            raw += t
    return {prefix + "_len": np.array(lens, dtype=np.uint32),
            prefix + "_kind": np.array(kinds, dtype=np.uint8),
            prefix + "_packed": np.concatenate(packed) if packed else np.zeros(0, dtype=np.uint8),
            prefix + "_raw": np.frombuffer(bytes(raw), dtype=np.uint8)}


def time_reference(ref: str, n_links: int, n_records: int, threads: int) -> None:
    from canu_amd.align_gfa import synth_graph
    job = synth_graph(seed=1, n_links=n_links, n_records=n_records)
    _, err, dt = run_reference(ref, "-T T.tigStore 2 -gfa -i in -o out".split(), job["utgs"], None,
                               job["gfa_text"], False, threads)
    print(f"reference alignGFA -gfa: {n_links} links, -t {threads}: {dt:.2f} s, "
          f"{n_links / dt:.1f} links/s;", err.strip().split("\n")[-2])
    _, err, dt = run_reference(ref, "-T T.tigStore 2 -C C.tigStore 2 -bed -i in -o out".split(),
                               job["utgs"], job["ctgs"], job["bed_text"], False, threads)
    print(f"reference alignGFA -bed: {n_records} records, -t {threads}: {dt:.2f} s, "
          f"{n_records / dt:.1f} records/s;", err.strip().split("\n")[-2])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--links", type=int, default=512)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--threads", type=int, default=1)
    a = ap.parse_args()
    tmp = None
    bd = a.build_dir
    if bd is None:
        tmp = tempfile.TemporaryDirectory()
        bd = tmp.name
    os.makedirs(bd, exist_ok=True)
    assert not os.path.abspath(bd).startswith(ROOT + os.sep), "build outside the repository"
    ref = build_reference(bd)
    if a.time:
        time_reference(ref, a.links, a.records, a.threads)
        return 0
    os.makedirs(a.out, exist_ok=True)
    for name, mk in FIXTURES:
        if a.only and name not in a.only.split(","):
            continue
        args, T, C, text = mk()
        out, err, _ = run_reference(ref, args, T, C, text, False)
        out_v, err_v, _ = run_reference(ref, args, T, C, text, True)
        arrays = tig_arrays("T", T)
        if C is not None:
            arrays.update(tig_arrays("C", C))
        path = os.path.join(a.out, f"gfa_{name}.npz")
        np.savez_compressed(
            path, args=np.frombuffer(" ".join(args).encode(), dtype=np.uint8),
            input=np.frombuffer(text.encode(), dtype=np.uint8),
            out=np.frombuffer(out.encode(), dtype=np.uint8),
            err=np.frombuffer(err.encode(), dtype=np.uint8),
            out_v=np.frombuffer(out_v.encode(), dtype=np.uint8),
            err_v=np.frombuffer(err_v.encode(), dtype=np.uint8), **arrays)
        print(path, os.path.getsize(path), "bytes;", err.strip().split("\n")[-2])
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
