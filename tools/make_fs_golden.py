#!/usr/bin/env python3
"""Write tests/golden/fs_*.npz from the reference falconsense.

    tools/make_fs_golden.py [--build-dir DIR] [--out tests/golden] [--only a,b]
    tools/make_fs_golden.py --time [--templates N] [--threads T]

The reference is compiled out of tree, into --build-dir (a temporary directory by default):
falconsense.C, falconConsensus*.C, generateCorrectionLayouts.C, tgStore.C, tgTig.C,
stashContains.C, edlib.C and AS_UTL_fasta.C with the oracle Makefile's REF_CXXFLAGS, linked with
the objects `make -C oracle` leaves in oracle/_ref/obj under --gc-sections.  Nothing of it is
committed.

Each job is run as canu runs it (CorrectReads.pm:503-512): the gkpStore by the reference's
gkStore code, the overlap store by its ovStore writer, the corStore by the reference
generateCorrectionLayouts (with a score file of zeros, so that no overlap is filtered), then
falconsense -G -C -b -e [-r] -cc -cl -ci.  A fixture holds the reads, the corStore's two files
as bytes, the layouts and children decoded from them, the options, the -r list, and the
reference's stdout and stderr.

  a  clean-ish reads (2 %), both orientations
  b  15 % error
  c  children with skips on both ends (askip, bskip), forward and reversed
  d  N bases; evidence longer than its template
  g  the reads of d, one template with N: a child trimmed below 500 (skipped) and a child of
     600 A against a stretch without A (rejected: distance / (end - start) >= 1)
  e  the reads of a with -r and a -b/-e range whose last read shows the exclusive end
  f  a template covered in two stretches (two pieces), thin templates (no piece), a template
     without children

--time runs the reference on the synthetic layouts of bench_fs.py (canu_amd.falconsense.
synth_layouts) and prints its wall time: the figure DESIGN.md sets beside bench_fs.py's.
"""
from __future__ import annotations

import argparse
import os
import re
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

import fs_restate as FS  # noqa: E402
import make_fe_golden as MG  # noqa: E402
from make_co_golden import MHC_SRCS, REF, ref_cxxflags  # noqa: E402

LIB_SRCS = ["correction/falconConsensus.C", "correction/falconConsensus-alignTag.C",
            "stores/tgStore.C", "stores/tgTig.C", "utgcns/stashContains.C",
            "overlapInCore/libedlib/edlib.C", "AS_UTL/AS_UTL_fasta.C"]
MAINS = {"fs_ref": "correction/falconsense.C", "gcl_ref": "correction/generateCorrectionLayouts.C"}
EXTRA_INC = ["correction", "utgcns", "overlapInCore/libedlib"]
HM = (1 << 21) - 1
UTG = 1 << 57                                         # forUTG: the store's filter keeps the overlap


def build_reference(build_dir: str) -> dict:
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    cxx = os.environ.get("CXX", "g++")
    flags = ref_cxxflags() + ["-I" + os.path.join(REF, "src", d) for d in EXTRA_INC]
    procs, objs = [], []
    for s in LIB_SRCS + list(MAINS.values()):
        o = os.path.join(build_dir, s.replace("/", "__") + ".o")
        procs.append(subprocess.Popen([cxx, *flags, "-c", os.path.join(REF, "src", s), "-o", o]))
        objs.append(o)
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("the reference did not compile")
    shared = objs[:len(LIB_SRCS)] + [os.path.join(obj, "fe_configure.o")]
    shared += [os.path.join(obj, s.replace("/", "__") + ".o") for s in MHC_SRCS]
    shared += [os.path.join(obj, "AS_UTL__AS_UTL_decodeRange.C.o"),
               os.path.join(obj, "AS_UTL__timeAndSize.C.o")]
    for o in shared:
        if not os.path.exists(o):
            raise FileNotFoundError(f"{o}: run `make -C oracle` first")
    out = {}
    for k, (name, _) in enumerate(MAINS.items()):
        out[name] = os.path.join(build_dir, name)
        subprocess.run([cxx, "-fopenmp", "-pthread", "-Wl,--gc-sections", "-o", out[name],
                        objs[len(LIB_SRCS) + k], *shared, "-lm"], check=True)
    return out


def encode_corstore(layouts, children) -> tuple[bytes, bytes]:
    """The two files of a version 1 corStore holding these layouts (tig IDs 0..max, the ones not
    given empty), in the format tests/fs_restate.py decodes."""
    by = {int(l["tig_id"]): l for l in layouts}
    n = max(by) + 1
    dat, tig = bytearray(), bytearray(struct.pack("<IIIII", FS.MASR_MAGIC, 1, n, 0, n))
    for t in range(n):
        l = by.get(t)
        llen, first, nch = (int(l["layout_len"]), int(l["first_child"]), int(l["n_children"])) \
            if l is not None else (0, 0, 0)
        rec = FS.TIG_RECORD.pack(t, 0.0, 0.0, 0, llen, 0, nch, 0)
        tig += rec + struct.pack("<Q", (1 << 14) | (len(dat) << 24))
        pos = np.zeros(nch, dtype=FS.POSITION)
        c = children[first:first + nch]
        pos["ident"], pos["flags"] = c["ident"], 1 | (c["reverse"] << 3)
        pos["anchor"], pos["min"], pos["max"] = t, c["min"], c["max"]
        pos["askip"], pos["bskip"] = c["askip"], c["bskip"]
        dat += b"TIGR" + rec + pos.tobytes()
    return bytes(tig), bytes(dat)


def run_reference(bins: dict, reads: list, recs: list, args: list, read_list=None,
                  corstore=None, threads: int = 1):
    """-> (tig bytes, dat bytes, stdout, stderr, seconds of falconsense)."""
    import oracle
    from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
    rs = MG.read_set(reads)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        gkp = oracle.build_gkpstore(rs, d)
        cor = os.path.join(d, "asm.corStore")
        if corstore is None:
            ovb = os.path.join(d, "in.ovb")
            write_ovb(np.array(recs, dtype=RECORD_DTYPE), ovb, counts=False)
            store = os.path.join(d, "asm.ovlStore")
            oracle.build_store(gkp, store, [ovb])
            scores = os.path.join(d, "scores")
            np.zeros(len(reads) + 1, dtype=np.uint16).tofile(scores)
            cp = subprocess.run([bins["gcl_ref"], "-G", gkp, "-O", store, "-S", scores, "-C", cor],
                                capture_output=True, text=True)
            if cp.returncode != 0:
                raise RuntimeError(f"generateCorrectionLayouts failed: {cp.stderr[-3000:]}")
        else:
            os.makedirs(cor)
            for name, raw in zip(("seqDB.v001.tig", "seqDB.v001.dat"), corstore):
                with open(os.path.join(cor, name), "wb") as f:
                    f.write(raw)
        with open(os.path.join(cor, "seqDB.v001.tig"), "rb") as f:
            tig = f.read()
        with open(os.path.join(cor, "seqDB.v001.dat"), "rb") as f:
            dat = f.read()
        cmd = [bins["fs_ref"], "-G", gkp, "-C", cor, "-t", str(threads), *args]
        if read_list is not None:
            lst = os.path.join(d, "readlist")
            with open(lst, "w") as f:
                f.write("".join(f"{i}\n" for i in read_list))
            cmd += ["-r", lst]
        t0 = time.time()
        cp = subprocess.run(cmd, capture_output=True)
        dt = time.time() - t0
        if cp.returncode != 0:
            raise RuntimeError(f"falconsense failed ({cp.returncode}): {cp.stderr[-3000:]!r}")
    return tig, dat, cp.stdout, cp.stderr, dt


CANU_ARGS = ["-cc", "4", "-cl", "500", "-ci", "0.5"]     # -ci goes through atoi there: 0


def _sample(seed, genome_len, n, err, lo, hi):
    S = MG.Sample(seed, genome_len, n, err, lo=lo, hi=hi)
    return S, S.all_pairs(10_000)


def fixture_a():
    S, recs = _sample(7101, 7000, 9, 0.02, 2200, 4500)
    return S.reads, recs, ["-b", "1", "-e", "10", *CANU_ARGS], None


def fixture_b():
    S, recs = _sample(7102, 6500, 9, 0.15, 2000, 4500)
    return S.reads, recs, ["-b", "1", "-e", "10", *CANU_ARGS], None


def fixture_c():
    """Every overlap shortened at both ends on both reads: the store keeps bhg5 / bhg3, which
    become askip / bskip."""
    S, recs = _sample(7103, 6000, 8, 0.06, 2200, 4200)
    out = []
    for k, (a, b, w0, w1) in enumerate(recs):
        cut5, cut3 = 40 + 17 * (k % 5), 25 + 31 * (k % 3)
        a5, a3 = (w0 & HM) + cut5, ((w0 >> 21) & HM) + cut3
        b5, b3 = (w1 & HM) + cut5, ((w1 >> 21) & HM) + cut3
        flip = (w0 >> 54) & 1
        if flip:                                       # B's ends are swapped under A's
            b5, b3 = (w1 & HM) + cut3, ((w1 >> 21) & HM) + cut5
        if a5 + a3 + 600 > len(S.reads[a - 1]) or b5 + b3 + 600 > len(S.reads[b - 1]):
            out.append((a, b, w0, w1))
            continue
        out.append((a, b, a5 | (a3 << 21) | (flip << 54) | UTG, b5 | (b3 << 21)))
    return S.reads, out, ["-b", "1", "-e", "9", *CANU_ARGS], None


def fixture_d(alone: bool = False):
    S, recs = _sample(7104, 5200, 7, 0.05, 2600, 4400)
    rng = S.rng
    # N bases.  The reference's reverse complement turns N into NUL and
    # its alignment-to-strings assertion then fails, so a tig with a reversed child that
    # holds an N cannot be run there: the -r list below leaves those tigs out.
    # Two reads get them: a forward read of the sample and the crafted template below.
    def with_n(seq: bytes) -> bytes:
        r = bytearray(seq)
        for p in rng.integers(50, len(r) - 50, 6):
            r[int(p)] = ord("N")
        r[1000:1003] = b"NNN"
        return bytes(r)
    first_fwd = next(i for i, w in enumerate(S.where) if w[2] == 0)
    S.reads[first_fwd] = with_n(S.reads[first_fwd])
    has_n = {first_fwd + 1}
    # a short template inside the genome whose overlaps claim no hang on the longer reads:
    # their evidence is longer than the template and is cut to it
    short = S.add(1500, 3600, 0, 0.04)
    for b in range(1, short):
        sb, eb, tb, _ = S.where[b - 1]
        if sb <= 1500 and eb >= 3600:
            recs.append((short, b, (int(tb) << 54) | UTG, 0))
    # a template with a stretch free of A, a child of 600 A placed there (rejected), and a
    # child trimmed to 450 bases (skipped)
    body = bytearray(S.genome[200:3400])
    body[1200:2100] = np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, 900)].tobytes()
    tmpl = S.add_raw(with_n(bytes(body)))
    has_n.add(tmpl)
    poly = S.add_raw(b"A" * 600)
    recs.append((tmpl, poly, 1350 | ((len(body) - 1950) << 21) | UTG, 0))
    stub = short - 1                                   # a sample read, 450 bases left by its skips
    assert stub not in has_n
    recs.append((tmpl, stub, ((len(body) - 450) << 21) | UTG,
                 (len(S.reads[stub - 1]) - 460) | (10 << 21)))
    for b in range(1, short):                          # and honest evidence for it
        r = None
        sb, eb, tb, pb = S.where[b - 1]
        lo, hi = max(sb, 200), min(eb, 3400)
        if hi - lo < 900 or any(x[0] == tmpl and x[1] == b for x in recs):
            continue
        blen = len(S.reads[b - 1])
        b_lo, b_hi = int(pb[lo - sb]), int(pb[hi - sb])
        a5, a3 = lo - 200, 3400 - hi
        b5, b3 = (b_lo, blen - b_hi) if tb == 0 else (blen - b_hi, b_lo)
        recs.append((tmpl, b, a5 | (a3 << 21) | (int(tb) << 54) | UTG, b5 | (b3 << 21)))
    unsafe = set()
    for (a, b, w0, _) in recs:
        if (w0 >> 54) & 1:
            unsafe |= ({a} if b in has_n else set()) | ({b} if a in has_n else set())
    keep = [t for t in range(1, len(S.reads) + 1) if t not in unsafe and t not in (poly, tmpl)]
    assert short in keep and any(t in has_n for t in keep) and tmpl not in unsafe
    if alone:
        return S.reads, recs, ["-b", str(tmpl), "-e", str(tmpl + 1), *CANU_ARGS], None
    return S.reads, recs, ["-b", "1", "-e", str(len(S.reads) + 1), *CANU_ARGS], keep


def fixture_g():
    """The crafted template of d by itself.  Run after other templates, the reference dies in it
    once one of its children is skipped; alone it does not."""
    return fixture_d(alone=True)


def fixture_e():
    reads, recs, _, _ = fixture_a()
    return reads, recs, ["-b", "2", "-e", "7", *CANU_ARGS], [1, 2, 4, 7, 9]


def fixture_f():
    S = MG.Sample(7106, 9000, 0, 0.04)
    # A read without overlaps: its layout is empty and carries the next read's length
    # (generateCorrectionLayouts.C:367-371).  It cannot come last: the reference then looks up
    # read UINT32_MAX and dies.
    S.add(7300, 8900, 0, 0.05)
    t1 = S.add(0, 4400, 0, 0.05)                       # covered at both ends only
    for k in range(6):
        S.add(0, 1700 + 20 * k, k & 1, 0.05)
        S.add(2750 - 20 * k, 4400, (k + 1) & 1, 0.05)
    t2 = S.add(4600, 7000, 1, 0.05)                    # two children: thin everywhere
    S.add(4600, 6800, 0, 0.05)
    S.add(4900, 7000, 1, 0.05)
    recs = [r for r in (S.record(a, b) for a in range(1, len(S.reads) + 1)
                        for b in range(a + 1, len(S.reads) + 1)) if r is not None]
    assert t1 == 2 and t2 == 15
    return S.reads, recs, ["-b", "1", "-e", str(len(S.reads) + 1), *CANU_ARGS], None


FIXTURES = [("a", fixture_a), ("b", fixture_b), ("c", fixture_c), ("d", fixture_d),
            ("e", fixture_e), ("f", fixture_f), ("g", fixture_g)]


def time_reference(bins: dict, n_templates: int, threads: int) -> None:
    from canu_amd.falconsense import synth_layouts
    reads, layouts, children = synth_layouts(n_templates)
    tig, dat = encode_corstore(layouts, children)
    args = ["-b", "1", "-e", str(n_templates + 1), *CANU_ARGS]
    _, _, out, _, dt = run_reference(bins, reads, [], args, corstore=(tig, dat), threads=threads)
    print(f"reference falconsense: {n_templates} templates, {int(layouts['n_children'].sum())} "
          f"children, -t {threads}: {dt:.2f} s, {n_templates / dt:.2f} templates/s, "
          f"{out.count(b'>')} corrected reads")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--templates", type=int, default=64)
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 1)
    a = ap.parse_args()
    tmp = None
    bd = a.build_dir
    if bd is None:
        tmp = tempfile.TemporaryDirectory()
        bd = tmp.name
    os.makedirs(bd, exist_ok=True)
    assert not os.path.abspath(bd).startswith(ROOT + os.sep), "build outside the repository"
    bins = build_reference(bd)
    if a.time:
        time_reference(bins, a.templates, a.threads)
        return 0
    os.makedirs(a.out, exist_ok=True)
    for name, mk in FIXTURES:
        if a.only and name not in a.only.split(","):
            continue
        reads, recs, args, rlist = mk()
        tig, dat, out, err, _ = run_reference(bins, reads, recs, args, rlist)
        layouts, children = FS.decode_corstore(tig, dat)
        rs = MG.read_set(reads)
        path = os.path.join(a.out, f"fs_{name}.npz")
        np.savez_compressed(
            path, bases=rs.bases, offsets=rs.offsets, lengths=rs.lengths,
            tig=np.frombuffer(tig, dtype=np.uint8), dat=np.frombuffer(dat, dtype=np.uint8),
            layouts=layouts, children=children,
            args=np.frombuffer(" ".join(args).encode(), dtype=np.uint8),
            read_list=np.array(rlist if rlist is not None else [], dtype=np.uint32),
            stdout=np.frombuffer(out, dtype=np.uint8), stderr=np.frombuffer(err, dtype=np.uint8))
        print(path, os.path.getsize(path), "bytes;", len(reads), "reads;",
              int(layouts["n_children"].sum()), "children;", out.count(b">"), "corrected reads;",
              len(re.findall(rb"Processing", err)), "templates")
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
