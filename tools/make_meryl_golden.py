#!/usr/bin/env python3
"""Write tests/golden/meryl_*.npz from the reference meryl and estimate-mer-threshold.

    tools/make_meryl_golden.py --meryl PATH --estimate PATH [--out tests/golden]

The two binaries are built by hand from the reference sources, outside this tree (DESIGN.md,
"Reference binaries for the k-mer count"); nothing of them is committed.  The inputs come from
fixed seeds, the command lines are canu's (Meryl.pm:434-470, :634), with a FASTA file in the
place of the gkpStore.  Each fixture holds the reads and the reference's output bytes only.
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

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _rc(b: bytes) -> bytes:
    return b.translate(_COMP)[::-1]


def reads_a() -> list[bytes]:
    """60 x 600 bp of a 3 kb genome, both strands, one read with NNN, one in lower case."""
    rng = np.random.default_rng(1601)
    g = _ACGT[rng.integers(0, 4, 3000)].tobytes()
    out = []
    for i in range(60):
        s = int(rng.integers(0, 3000 - 600 + 1))
        r = g[s:s + 600]
        if rng.random() < 0.5:
            r = _rc(r)
        out.append(r)
    out[7] = out[7][:250] + b"NNN" + out[7][253:]
    out[11] = out[11].lower()
    return out


def reads_b() -> list[bytes]:
    """300 x 2 kb at ~20x of a 30 kb genome; a 400-bp repeat written into 40 reads."""
    rng = np.random.default_rng(2201)
    g = _ACGT[rng.integers(0, 4, 30000)].tobytes()
    rep = _ACGT[rng.integers(0, 4, 400)].tobytes()
    out = []
    for i in range(300):
        s = int(rng.integers(0, 30000 - 2000 + 1))
        r = bytearray(g[s:s + 2000])
        for p in np.nonzero(rng.random(2000) < 0.01)[0]:     # 1 % substitutions
            r[p] = b"ACGT"[(b"ACGT".index(r[p]) + int(rng.integers(1, 4))) % 4]
        r = bytes(r)
        if i < 40:
            p = int(rng.integers(0, 1600))
            r = r[:p] + rep + r[p + 400:]
        if rng.random() < 0.5:
            r = _rc(r)
        out.append(r)
    return out


def reads_c() -> list[bytes]:
    """Low complexity: homopolymers, dinucleotide repeats, palindromic 16-mers, reads shorter
    than k and of exactly k (k = 16), an all-N read, an empty read."""
    rng = np.random.default_rng(1603)
    out = [b"A" * 5000] * 20 + [b"T" * 5000] * 20
    out += [b"AC" * 1500, b"CA" * 1200 + b"C", b"GT" * 900]
    pal = []
    for _ in range(12):                      # x + revcomp(x) is its own reverse complement
        h = _ACGT[rng.integers(0, 4, 8)].tobytes()
        pal.append(h + _rc(h))
    out.append(b"".join(pal))
    out += [b"ACGTACGTAC", b"ACGGTCATGCAATGCC", b"ACGTACGTACGTACGT", b"N" * 300, b"",
            b"acgtnACGTTTGACCATGACAGTACCCATnnACG"]
    return out


def write_fasta(path: str, reads: list[bytes]) -> None:
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n" % i + r + b"\n")


def run_meryl(meryl: str, reads: list[bytes], k: int, thresholds: list[int]) -> dict:
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fasta")
        write_fasta(fa, reads)
        db = os.path.join(d, f"asm.ms{k}")
        subprocess.run([meryl, "-B", "-C", "-L", "2", "-v", "-m", str(k), "-threads", "4",
                        "-memory", "1024", "-s", fa, "-o", db + ".WORKING"], check=True,
                       cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(db + ".WORKING.mcdat", db + ".mcdat")
        os.replace(db + ".WORKING.mcidx", db + ".mcidx")
        h = subprocess.run([meryl, "-Dh", "-s", db], check=True, cwd=d, capture_output=True)
        out = {"histogram": h.stdout, "info": h.stderr}
        for t in thresholds:
            p = subprocess.run([meryl, "-Dt", "-n", str(t), "-s", db], check=True, cwd=d,
                               capture_output=True)
            out[f"dt_{t}"] = p.stdout
    return out


def run_estimate(estimate: str, hist: bytes, cov: float) -> tuple[bytes, bytes]:
    with tempfile.TemporaryDirectory() as d:
        hp = os.path.join(d, "asm.histogram")
        with open(hp, "wb") as f:
            f.write(hist)
        c = ("%g" % cov)
        p = subprocess.run([estimate, "-h", hp, "-c", c], check=True, capture_output=True)
    return p.stdout, p.stderr


def _rows(pairs) -> bytes:
    """Histogram rows in meryl -Dh's layout from (count, distinct) pairs."""
    nd = sum(n for _, n in pairs)
    nt = sum(c * n for c, n in pairs)
    d = t = 0
    out = []
    for c, n in pairs:
        d += n
        t += c * n
        out.append("%d\t%d\t%.4f\t%.4f\n" % (c, n, d / nd, t / nt))
    return "".join(out).encode()


def synthetic_histograms() -> dict[str, bytes]:
    """One histogram per way out of estimate-mer-threshold's loops (which one a case takes
    shows in the recorded stderr)."""
    # every count up to 400 populated: the sliding window never empties ("No break")
    nobreak = [(1, 90000)] + [(c, max(3, int(4000 * np.exp(-((c - 30) / 9.0) ** 2)) + 5))
                              for c in range(2, 400)]
    # a coverage bump, a gap, then one count holding 10x the window's mean
    jump = [(1, 50000)] + [(c, int(3000 * np.exp(-((c - 20) / 5.0) ** 2)) + 1)
                           for c in range(2, 60)] + [(c, 2) for c in range(60, 140)] + \
           [(140, 900)] + [(c, 1) for c in range(141, 200)]
    # most of the sequence in high counts: the 90 % rule stops the scan under a small -c
    ninety = [(1, 20000)] + [(c, 400) for c in range(2, 40)] + \
             [(c, 60) for c in range(40, 600)] + [(c, 3) for c in range(600, 900)]
    # hist[kk] * kk beyond 2^32: the products wrap
    wrap = [(1, 3000000000)] + [(c, 1500000000 // c + 7) for c in range(2, 90)] + \
           [(c, 90000000) for c in range(90, 160)]
    # a bump, then nothing for longer than the window, then a lone high count ("Found break")
    gap = [(1, 50000)] + [(c, int(3000 * np.exp(-((c - 20) / 5.0) ** 2)) + 1)
                          for c in range(2, 41)] + [(500, 3), (501, 1)]
    return {"syn_gap": _rows(gap), "syn_nobreak": _rows(nobreak), "syn_jump": _rows(jump),
            "syn_ninety": _rows(ninety), "syn_wrap": _rows(wrap)}


def pack_reads(reads: list[bytes]) -> dict:
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    if len(reads) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return {"bases": np.frombuffer(b"".join(reads), dtype=np.uint8), "offsets": offs,
            "lengths": lens}


def _bytes(b: bytes) -> np.ndarray:
    return np.frombuffer(b, dtype=np.uint8)


COVERAGES = [0, 1, 5, 30]
FIXTURES = [("a", reads_a, 16, [1, 2, 5, 12]), ("a", reads_a, 5, [2, 200]),
            ("a", reads_a, 31, [2, 5]), ("a", reads_a, 32, [2, 5]),
            ("b", reads_b, 22, [10, 25, 41]), ("c", reads_c, 16, [1, 2, 100])]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--meryl", required=True)
    ap.add_argument("--estimate", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    hists: dict[str, bytes] = {}
    for name, mk, k, thr in FIXTURES:
        reads = mk()
        texts = run_meryl(os.path.abspath(a.meryl), reads, k, thr)
        if k in (16, 22):
            hists[f"{name}_k{k}"] = texts["histogram"]
        arrs = pack_reads(reads)
        arrs["k"] = np.array([k], dtype=np.uint32)
        arrs["thresholds"] = np.array(thr, dtype=np.uint64)
        for key, val in texts.items():
            arrs[key] = _bytes(val)
        path = os.path.join(a.out, f"meryl_{name}_k{k}.npz")
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    hists.update(synthetic_histograms())
    arrs = {"names": np.array(sorted(hists)), "coverages": np.array(COVERAGES, dtype=np.float64)}
    for name in sorted(hists):
        arrs[f"{name}__hist"] = _bytes(hists[name])
        for c in COVERAGES:
            so, se = run_estimate(os.path.abspath(a.estimate), hists[name], c)
            arrs[f"{name}__out_{c}"] = _bytes(so)
            arrs[f"{name}__err_{c}"] = _bytes(se)
            print(name, "-c", c, "->", so.decode().strip(),
                  [l for l in se.decode().split("\n") if "break" in l])
    path = os.path.join(a.out, "meryl_emt.npz")
    np.savez_compressed(path, **arrs)
    print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
