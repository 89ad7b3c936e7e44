#!/usr/bin/env python3
"""Write tests/golden/pair_*.npz from the reference overlapPair.

    tools/make_pair_golden.py --overlapPair PATH [--out tests/golden]

The binary is built by hand from the reference sources, outside this tree (DESIGN.md,
"Reference binary for overlapPair"); nothing of it is committed.  Reads and input overlaps come
from fixed seeds; the gkpStore is written by the reference's own gkStore code
(oracle.build_gkpstore), the input .ovb by this project's writer, and the command line is
canu's (OverlapMhap.pm:524-534).  Each fixture holds the reads, the input records, the
reference's output records (read back with its own ovFile reader), the counters of
alignStats::reportFinal and the argument line.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

COUNTERS = ("nSkipped", "nPassed", "nFailed", "nFailExtA", "nFailExtB", "nFailExt", "nPartial",
            "nDovetail", "nExt5a", "nExt3a", "nExt5b", "nExt3b")


def _rc(b: bytes) -> bytes:
    return b.translate(_COMP)[::-1]


def _mutate(rng, seg: bytes, err: float) -> bytes:
    """Substitutions, insertions and deletions, a third each."""
    out = bytearray()
    for c in seg:
        u = rng.random()
        if u < err / 3:
            out.append(b"ACGT"[(b"ACGT".index(c) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * err / 3:
            out.append(c)
            out.append(b"ACGT"[int(rng.integers(0, 4))])
        elif u < err:
            continue
        else:
            out.append(c)
    return bytes(out)


class Sample:
    """Reads cut from one genome, with where they came from."""

    def __init__(self, seed: int, genome_len: int, n_reads: int, err: float,
                 lo: int = 1500, hi: int = 3000):
        self.rng = rng = np.random.default_rng(seed)
        self.genome = _ACGT[rng.integers(0, 4, genome_len)].tobytes()
        self.reads: list[bytes] = []
        self.where: list[tuple[int, int, int]] = []       # genome start, end, strand
        for _ in range(n_reads):
            L = int(rng.integers(lo, hi + 1))
            s = int(rng.integers(0, genome_len - L + 1))
            self.add(s, s + L, int(rng.integers(0, 2)), err)

    def add(self, s: int, e: int, strand: int, err: float) -> int:
        r = _mutate(self.rng, self.genome[s:e], err)
        self.reads.append(_rc(r) if strand else r)
        self.where.append((s, e, strand))
        return len(self.reads)                              # its read ID

    def add_raw(self, seq: bytes) -> int:
        self.reads.append(seq)
        self.where.append((-1, -1, 0))
        return len(self.reads)

    def record(self, a: int, b: int, jitter: int = 300, min_true: int = 600):
        """The overlap of reads a, b (IDs) as MHAP would report it: the true hangs moved by up
        to +-jitter bases each.  None if the reads share fewer than min_true genome bases."""
        rng = self.rng
        sa, ea, ta = self.where[a - 1]
        sb, eb, tb = self.where[b - 1]
        lo, hi = max(sa, sb), min(ea, eb)
        if hi - lo < min_true:
            return None
        alen, blen = len(self.reads[a - 1]), len(self.reads[b - 1])
        if ta == 0:
            a5, a3, b5, b3 = lo - sa, ea - hi, lo - sb, eb - hi
        else:
            a5, a3, b5, b3 = ea - hi, lo - sa, eb - hi, lo - sb
        h = [a5, a3, b5, b3]
        if jitter:
            h = [v + int(rng.integers(-jitter, jitter + 1)) for v in h]
        return fit_record(a, b, h, alen, blen, ta != tb)


def fit_record(a, b, h, alen, blen, flipped):
    """Hangs clipped so that each read keeps a span of at least one base."""
    a5 = min(max(h[0], 0), alen - 1)
    a3 = min(max(h[1], 0), alen - 1 - a5)
    b5 = min(max(h[2], 0), blen - 1)
    b3 = min(max(h[3], 0), blen - 1 - b5)
    w0 = a5 | (a3 << 21) | (int(bool(flipped)) << 54)
    w1 = b5 | (b3 << 21)
    return (a, b, w0, w1)


def all_pairs(S: Sample, limit: int, jitter: int = 300):
    recs = []
    n = len(S.reads)
    for a in range(1, n + 1):
        for b in range(a + 1, n + 1):
            r = S.record(a, b, jitter)
            if r is not None:
                recs.append(r)
    S.rng.shuffle(recs)
    return recs[:limit]


def fixture_a():
    S = Sample(4101, 24000, 70, 0.012)
    return S.reads, all_pairs(S, 300), ["-len", "500", "-erate", "0.045"]


def fixture_b():
    S = Sample(4102, 20000, 50, 0.08)
    return S.reads, all_pairs(S, 220), ["-partial", "-len", "500", "-erate", "0.30"]


def fixture_c():
    S = Sample(4103, 20000, 50, 0.04)
    return S.reads, all_pairs(S, 220), ["-len", "500", "-erate", "0.144", "-invert"]


def fixture_d():
    """The edge set; every kind once with B forward and once with B flipped."""
    S = Sample(4104, 16000, 24, 0.01)
    rng = S.rng
    recs = all_pairs(S, 60)
    G = S.genome
    for strand_b in (0, 1):
        # spans below -len, and a pair that shares too little
        a = S.add(1000, 3000, 0, 0.01)
        b = S.add(2700, 4700, strand_b, 0.01)
        recs.append(fit_record(a, b, [1700, 0, 0, 1700],
                               len(S.reads[a - 1]), len(S.reads[b - 1]), strand_b))
        recs.append(fit_record(a, b, [1800, 0, 0, 1600], len(S.reads[a - 1]),
                               len(S.reads[b - 1]), strand_b))
        # unrelated reads: every alignment fails
        u = S.add_raw(_ACGT[rng.integers(0, 4, 2000)].tobytes())
        v = S.add_raw(_ACGT[rng.integers(0, 4, 2200)].tobytes())
        recs.append(fit_record(u, v, [900, 0, 0, 1100], 2000, 2200, strand_b))
        recs.append(fit_record(u, a, [0, 0, 0, 0], 2000, len(S.reads[a - 1]), strand_b))
        # one side failing only: B's claimed span is most of the read, the truth 700 bases
        a = S.add(5000, 7500, 0, 0.01)
        b = S.add(6800, 9300, strand_b, 0.01)
        al, bl = len(S.reads[a - 1]), len(S.reads[b - 1])
        recs.append(fit_record(a, b, [1800, 0, 0, 200], al, bl, strand_b))
        recs.append(fit_record(a, b, [300, 0, 0, 1800], al, bl, strand_b))
        # contained: B inside A, A inside B, exact and perturbed
        a = S.add(9000, 12000, 0, 0.01)
        b = S.add(9600, 11400, strand_b, 0.01)
        for j in (0, 150, 300):
            recs.append(S.record(a, b, j))
        c = S.add(9600, 11400, 0, 0.01)
        d = S.add(9000, 12000, strand_b, 0.01)
        for j in (0, 200):
            recs.append(S.record(c, d, j))
        # each dovetail extension: true dovetails whose reported hangs stop short of the ends
        a = S.add(2000, 4500, 0, 0.01)
        b = S.add(3500, 6000, strand_b, 0.01)
        al, bl = len(S.reads[a - 1]), len(S.reads[b - 1])
        for h in ([1700, 150, 180, 1650], [1650, 10, 120, 1500], [1550, 120, 30, 1700]):
            recs.append(fit_record(a, b, h, al, bl, strand_b))
        a = S.add(3500, 6000, 0, 0.01)
        b = S.add(2000, 4500, strand_b, 0.01)
        al, bl = len(S.reads[a - 1]), len(S.reads[b - 1])
        for h in ([160, 1700, 1650, 140], [30, 1600, 1500, 170]):
            recs.append(fit_record(a, b, h, al, bl, strand_b))
        # a failed extension that restores: the reads' ends are not from the genome
        ja = _ACGT[rng.integers(0, 4, 350)].tobytes()
        jb = _ACGT[rng.integers(0, 4, 350)].tobytes()
        ra = _mutate(rng, G[12000:14000], 0.01) + ja
        rb = jb + _mutate(rng, G[12900:14900], 0.01)
        a = S.add_raw(ra)
        b = S.add_raw(_rc(rb) if strand_b else rb)
        recs.append(fit_record(a, b, [900, 350, 350, 900], len(ra), len(rb), strand_b))
        recs.append(fit_record(a, b, [1000, 500, 500, 1000], len(ra), len(rb), strand_b))
        # N runs on both sides
        ra = bytearray(_mutate(rng, G[1000:3200], 0.01))
        rb = bytearray(_mutate(rng, G[1900:4100], 0.01))
        ra[1500:1520] = b"N" * 20
        ra[63:65] = b"NN"
        rb[300:330] = b"N" * 30
        rb[1000:1001] = b"N"
        a = S.add_raw(bytes(ra))
        b = S.add_raw(_rc(bytes(rb)) if strand_b else bytes(rb))
        recs.append(fit_record(a, b, [850, 50, 40, 870], len(ra), len(rb), strand_b))
        recs.append(fit_record(a, b, [1000, 0, 0, 800], len(ra), len(rb), strand_b))
        # ties: a homopolymer pair and a period-3 pair
        a = S.add_raw(b"A" * 1800)
        b = S.add_raw((b"T" if strand_b else b"A") * 2100)
        recs.append(fit_record(a, b, [600, 0, 0, 900], 1800, 2100, strand_b))
        recs.append(fit_record(a, b, [0, 200, 300, 0], 1800, 2100, strand_b))
        a = S.add_raw(b"ACG" * 600)
        pb = b"ACG" * 700
        b = S.add_raw(_rc(pb) if strand_b else pb)
        recs.append(fit_record(a, b, [700, 0, 0, 1000], 1800, 2100, strand_b))
        recs.append(fit_record(a, b, [100, 200, 301, 2], 1800, 2100, strand_b))
    recs = [r for r in recs if r is not None]
    return S.reads, recs, ["-len", "500", "-erate", "0.06"]


FIXTURES = [("a", fixture_a), ("b", fixture_b), ("c", fixture_c), ("d", fixture_d)]


def read_set(reads: list[bytes]):
    from canu_amd.synth import ReadSet
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    if len(reads) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return ReadSet(bases=np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets=offs,
                   lengths=lens, first_iid=1)


def run_reference(binary: str, reads, recs, args):
    import oracle
    from pair_restate import parse_report
    from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
    rs = read_set(reads)
    inp = np.array(recs, dtype=RECORD_DTYPE)
    with tempfile.TemporaryDirectory() as d:
        gkp = oracle.build_gkpstore(rs, d)
        os.makedirs(os.path.join(d, "results"))
        src = os.path.join(d, "results", "000001.mhap.ovb")
        dst = os.path.join(d, "results", "000001.WORKING.ovb")
        write_ovb(inp, src, counts=False)
        line = ["-G", gkp, "-O", src, "-o", dst, *args, "-memory", "4", "-t", "2"]
        p = subprocess.run([binary, *line], capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"overlapPair failed ({p.returncode}): {p.stderr[-2000:]}")
        out = oracle.read_ovb_reference(dst)
        left = sorted(os.listdir(os.path.join(d, "results")))
    return rs, inp, out, parse_report(p.stderr), left


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--overlapPair", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name, mk in FIXTURES:
        reads, recs, args = mk()
        rs, inp, out, counters, left = run_reference(os.path.abspath(a.overlapPair), reads, recs,
                                                     args)
        assert out.shape == inp.shape
        path = os.path.join(a.out, f"pair_{name}.npz")
        np.savez_compressed(
            path, bases=rs.bases, offsets=rs.offsets, lengths=rs.lengths,
            **{"in_" + f: inp[f] for f in inp.dtype.names},
            **{"out_" + f: out[f] for f in out.dtype.names},
            counters=np.array([counters[k] for k in COUNTERS], dtype=np.uint64),
            args=np.frombuffer(" ".join(args).encode(), dtype=np.uint8))
        print(path, os.path.getsize(path), "bytes;", len(recs), "overlaps;", counters)
        print("   files the reference left:", left)
    return 0


if __name__ == "__main__":
    sys.exit(main())
