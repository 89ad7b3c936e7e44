#!/usr/bin/env python3
"""Write tests/golden/co_*.npz from the reference correctOverlaps.

    tools/make_co_golden.py [--correctOverlaps PATH] [--build-dir DIR] [--out tests/golden]

Without --correctOverlaps the reference is compiled out of tree, into --build-dir (a temporary
directory by default): its five correctOverlaps*.C files with the oracle Makefile's
REF_CXXFLAGS, linked with the objects `make -C oracle` leaves in oracle/_ref/obj (fe_configure.o
for AS_configure, the stores, timeAndSize and Binomial_Bound).  Nothing of it is committed.

Each job is run as canu runs it (OverlapErrorAdjustment.pm:509-517): the gkpStore by the
reference's gkStore code, the overlap store by its ovStore writer, the .red file by the reference
findErrors (oracle/_ref/fe_ref) over reads 1..N.  The overlaps carry distinct nonzero evalues,
so a failed overlap shows the one it kept.  Each fixture holds the reads, the store's records
of the range in store order, the .red bytes, the reference's .oea bytes, its nine counters and
the numbers of its "Corrected" line, the range and the options.

  a  utg-like reads at 0.045           b  noisy reads at 0.144 (the one with natural inserts)
  c  the vote lab "f" of tests/fe_votes.py -- inserts, deletes and substitution-then-insert at
     one base -- over all its reads, so that the store's twins bring the corrected reads in as
     B in both orientations, with probes whose hangs land one short of, on and one past an
     adjust position of the A list, the forward B list and the reverse B list
  d  the edge set: an N read, reads without corrections, hangs of 0, B reads outside the
     range
  e  planted leading gaps for both trims
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import co_restate as CR  # noqa: E402
import fe_restate as FR  # noqa: E402
import fe_votes as FV  # noqa: E402
import make_fe_golden as MG  # noqa: E402

REF = os.environ.get("CANU_REFERENCE", "/root/reference")
CO_SRCS = ["correctOverlaps.C", "correctOverlaps-Correct_Frags.C",
           "correctOverlaps-Prefix_Edit_Distance.C", "correctOverlaps-Read_Olaps.C",
           "correctOverlaps-Redo_Olaps.C"]
MHC_SRCS = ["stores/gkStore.C", "stores/gkStoreEncode.C", "stores/ovOverlap.C", "stores/ovStore.C",
            "stores/ovStoreWriter.C", "stores/ovStoreFilter.C", "stores/ovStoreFile.C",
            "stores/ovStoreHistogram.C", "stores/libsnappy/snappy-sinksource.cc",
            "stores/libsnappy/snappy-stubs-internal.cc", "stores/libsnappy/snappy.cc",
            "AS_UTL/AS_UTL_fileIO.C", "AS_UTL/AS_UTL_reverseComplement.C"]


def ref_cxxflags() -> list[str]:
    """REF_CXXFLAGS of oracle/Makefile."""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    flags = re.search(r"^REF_CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(RS)", os.path.join(REF, "src")).split()


def build_reference(build_dir: str) -> str:
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    src = os.path.join(REF, "src", "overlapErrorAdjustment")
    cxx = os.environ.get("CXX", "g++")
    objs = []
    for s in CO_SRCS:
        o = os.path.join(build_dir, s + ".o")
        subprocess.run([cxx, *ref_cxxflags(), "-c", os.path.join(src, s), "-o", o], check=True)
        objs.append(o)
    objs.append(os.path.join(obj, "fe_configure.o"))
    objs += [os.path.join(obj, s.replace("/", "__") + ".o") for s in MHC_SRCS]
    objs += [os.path.join(obj, "AS_UTL__timeAndSize.C.o"),
             os.path.join(obj, "overlapInCore__liboverlap__Binomial_Bound.C.o")]
    for o in objs:
        if not os.path.exists(o):
            raise FileNotFoundError(f"{o}: run `make -C oracle` first")
    out = os.path.join(build_dir, "co_ref")
    subprocess.run([cxx, "-fopenmp", "-pthread", "-Wl,--gc-sections", "-o", out, *objs, "-lm"],
                   check=True)
    return out


def number(recs: list) -> list:
    """Distinct nonzero evalues."""
    assert len(recs) < CR.AS_MAX_EVALUE
    return [CR.with_evalue(tuple(r), 1 + k) for k, r in enumerate(recs)]


COUNTER_RE = (r"Olaps Fwd (\d+)", r"Olaps Rev (\d+)", r"Total:\s+(\d+)", r"Failed: (\d+) \(both\)",
              r"Failed: (\d+) \(either\)", r"Failed: (\d+) \(match to end\)",
              r"Failed: (\d+) \(negative length\)", r"rhaFail (\d+)", r"rhaPass (\d+)")
CORRECTED_RE = r"Corrected (\d+) bases with (\d+) substitutions, (\d+) deletions and (\d+) insertions"


def run_reference(binary, reads, fe_recs, co_recs, bgn, end, fe_args, erate):
    """-> (rs, the store's records of [bgn, end], .red bytes, .oea bytes, the 13 counters)."""
    import oracle
    from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
    rs = MG.read_set(reads)
    n = len(reads)
    red, _, _, _ = oracle.run_find_errors(rs, np.array(fe_recs, dtype=RECORD_DTYPE), 1, n, fe_args)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        gkp = oracle.build_gkpstore(rs, d)
        ovb = os.path.join(d, "in.ovb")
        write_ovb(np.array(co_recs, dtype=RECORD_DTYPE), ovb, counts=False)
        store = os.path.join(d, "asm.ovlStore")
        oracle.build_store(gkp, store, [ovb])
        stored = oracle.dump_store(gkp, store)
        redf = os.path.join(d, "red.red")
        with open(redf, "wb") as f:
            f.write(red)
        oea = os.path.join(d, "00001.oea")
        cp = subprocess.run([binary, "-G", gkp, "-O", store, "-R", str(bgn), str(end), "-e",
                             repr(erate), "-l", "500", "-c", redf, "-o", oea],
                            capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"correctOverlaps failed ({cp.returncode}): {cp.stderr[-3000:]}")
        with open(oea, "rb") as f:
            raw = f.read()
    cnt = [int(re.search(p, cp.stderr).group(1)) for p in COUNTER_RE]
    cnt += [int(v) for v in re.search(CORRECTED_RE, cp.stderr).groups()]
    sel = stored[(stored["a"] >= bgn) & (stored["a"] <= end)]
    return rs, sel, red, raw, cnt


def fixture_a():
    reads, recs, bgn, end, args = MG.fixture_a()
    recs = number(recs)
    return reads, recs, recs, bgn, end, args, 0.045


def fixture_b():
    reads, recs, bgn, end, args = MG.fixture_b()
    recs = number(recs)
    return reads, recs, recs, bgn, end, args, 0.144


def fixture_c():
    """Lab "f" and the probes.  The probes need the adjust lists, which need the .red file of
    reads 1..N on what the store holds (the lab's overlaps and their twins): the restatement of
    findErrors gives it here (tests/test_fe_cpu.py pins it to the reference on this very lab),
    and main() checks that the reference wrote the same."""
    from canu_amd.find_errors import store_view
    from canu_amd.overlap_in_core import RECORD_DTYPE
    lab = FV.fixture("f")
    reads, recs, _, n_a = lab.job()
    n = len(reads)
    view = store_view(np.array(recs, dtype=RECORD_DTYPE))
    red, _, _ = FR.find_errors(view, {i + 1: r for i, r in enumerate(reads)}, 1, n, lab.P)
    # Correct_Frags sizes its one array of corrected bases by the reads as stored
    # (correctOverlaps-Correct_Frags.C:226-230, :251): a range whose insertions outnumber its
    # deletions writes past it and the reference dies in free().  The range starts at the first
    # read from which on they do not; the reads before it still come in as B reads.
    t = (red["word"] >> 2) & 15
    net = np.zeros(n + 2, dtype=np.int64)
    np.add.at(net, red["readID"][t >= FR.A_INSERT], 1)
    np.add.at(net, red["readID"][t == FR.DELETE], -1)
    tail = np.cumsum(net[::-1])[::-1]
    bgn = int(np.nonzero(tail[1:] <= 0)[0][0]) + 1
    assert bgn < n_a and (t[red["readID"] >= bgn] >= FR.A_INSERT).any()
    probes = []
    taken = {"a": 0, "bf": 0, "br": 0}
    for rid in range(1, n_a + 1):
        seq, fadj, _ = CR.correct_read(rid, FR.filter_read(reads[rid - 1]), red, 0)
        if not fadj:
            continue
        radj = CR.make_rev_adjust(fadj, seq.shape[0])
        other = n_a + 1 + (rid % (n - n_a))               # a piece: in the range, not this read
        for which, lst in (("a", fadj), ("bf", fadj), ("br", radj)):
            if taken[which] >= 4 or (which == "a" and rid < bgn):
                continue
            taken[which] += 1
            pos = lst[len(lst) // 2][0]
            for d in (-1, 0, 1):
                h = pos + d
                if h <= 0 or h >= len(reads[rid - 1]) - 8:
                    continue
                if which == "a":
                    probes.append(FR.make_record(rid, other, h, 10, len(probes) & 1))
                else:
                    probes.append(FR.make_record(other, rid, -h, 10, which == "br"))
    assert all(taken[w] >= 2 for w in taken), taken
    return reads, recs, number(recs + probes), bgn, n, lab.args, 0.06, red


def planted_trims(S, recs) -> None:
    """A read with leading bases its partner lacks, and the mirror case; each with the recorded
    hang at, below and above the length of the gap (the trims' i == stop, both ways, and
    i < stop).  The run of T cannot match: the partner starts with another letter."""
    rng, G = S.rng, S.genome
    at = 100
    for fl in (0, 1):
        o = MG._rc if fl else (lambda s: s)
        for case, (lead, later_gap) in enumerate(((2, False), (10, True), (10, False))):
            core = bytearray(G[at:at + 420])
            at += 450
            if core[0] == ord("T"):
                core[0] = ord("A")
            long_side = bytearray(core) + MG._rand(rng, 60)
            if later_gap:
                del long_side[200]
            pre = MG._rand(rng, lead)
            x = S.add_raw(pre + b"TTT" + bytes(core))                  # the extra bases on A
            y = S.add_raw(o(bytes(long_side)))
            recs.append(FR.make_record(x, y, lead, 60, fl))
            x2 = S.add_raw(bytes(long_side))                          # the extra bases on B
            y2 = S.add_raw(o(pre + b"TTT" + bytes(core)))
            recs.append(FR.make_record(x2, y2, -lead, -60, fl))


def fixture_d():
    reads, recs, bgn, end, args = MG.fixture_d()
    recs = number(recs)
    return reads, recs, recs, bgn, end, args, 0.06


def fixture_e():
    class S:
        rng = np.random.default_rng(5204)
        reads: list = []

        @classmethod
        def add_raw(cls, seq):
            cls.reads.append(bytes(seq))
            return len(cls.reads)
    S.genome = MG._rand(S.rng, 12000)
    recs: list = []
    planted_trims(S, recs)
    recs = number(recs)
    return S.reads, recs, recs, 1, len(S.reads), ["-e", "0.06"], 0.06


FIXTURES = [("a", fixture_a), ("b", fixture_b), ("c", fixture_c), ("d", fixture_d),
            ("e", fixture_e)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--correctOverlaps", default=None)
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    tmp = None
    binary = a.correctOverlaps
    if binary is None:
        bd = a.build_dir
        if bd is None:
            tmp = tempfile.TemporaryDirectory()
            bd = tmp.name
        os.makedirs(bd, exist_ok=True)
        assert not os.path.abspath(bd).startswith(ROOT + os.sep), "build outside the repository"
        binary = build_reference(bd)
    for name, mk in FIXTURES:
        made = mk()
        reads, fe_recs, co_recs, bgn, end, fe_args, erate = made[:7]
        rs, sel, red, oea, cnt = run_reference(os.path.abspath(binary), reads, fe_recs, co_recs,
                                               bgn, end, fe_args, erate)
        if len(made) > 7:
            assert np.frombuffer(red, dtype=FR.RED_DTYPE).tobytes() == made[7].tobytes(), \
                "the probes were placed on another .red than the reference's"
        path = os.path.join(a.out, f"co_{name}.npz")
        np.savez_compressed(
            path, bases=rs.bases, offsets=rs.offsets, lengths=rs.lengths,
            **{"in_" + f: sel[f] for f in sel.dtype.names},
            red=np.frombuffer(red, dtype=np.uint8), oea=np.frombuffer(oea, dtype=np.uint8),
            counters=np.array(cnt + [bgn, end], dtype=np.uint64),
            args=np.frombuffer(f"-e {erate!r}".encode(), dtype=np.uint8))
        print(path, os.path.getsize(path), "bytes;", sel.shape[0], "overlaps;",
              dict(zip(CR.COUNTERS + CR.CORRECTED, cnt)))
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
