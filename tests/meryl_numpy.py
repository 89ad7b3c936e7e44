"""A short numpy restatement of `meryl -B [-C] -L low -m k` and its two dump texts (helper
module, not a test).  test_meryl_cpu.py pins it to the reference's golden texts byte for
byte; the GPU tests then compare the device count against it."""
from __future__ import annotations

import os
import struct
import types

import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i                  # lower case counts as upper case


def all_mers(bases, offsets, lengths, k: int, canonical: bool = True) -> np.ndarray:
    """Every mer of every read as a 2-bit number (first base most significant): no mer spans
    two reads or a non-ACGT byte; canonical = min(mer, reverse complement)."""
    out = []
    mask = np.uint64((1 << (2 * k)) - 1) if k < 32 else np.uint64(0xFFFFFFFFFFFFFFFF)
    for o, n in zip(offsets.tolist(), lengths.tolist()):
        if n < k:
            continue
        c = _CODE[np.asarray(bases[o:o + n])]
        m = n - k + 1
        bad = np.concatenate([[0], np.cumsum(c > 3)])
        ok = (bad[k:] - bad[:-k]) == 0
        c = (c & 3).astype(np.uint64)
        f = np.zeros(m, dtype=np.uint64)
        r = np.zeros(m, dtype=np.uint64)
        for i in range(k):
            f = (f << np.uint64(2)) | c[i:i + m]
            r = r | ((np.uint64(3) - c[i:i + m]) << np.uint64(2 * i))
        f &= mask
        key = np.minimum(f, r) if canonical else f
        out.append(key[ok])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


class Counts:
    """mers/counts: every distinct mer, ascending; hist[c] = distinct mers with count c."""

    def __init__(self, keys: np.ndarray, k: int, low_count: int = 2):
        self.k, self.low_count = k, low_count
        self.all_mers, self.all_counts = np.unique(keys, return_counts=True)
        self.total = int(keys.shape[0])
        self.distinct = int(self.all_mers.shape[0])
        self.unique = int((self.all_counts == 1).sum())
        self.largest = int(self.all_counts.max()) if self.distinct else 0
        self.hist = np.bincount(self.all_counts, minlength=self.largest + 1).astype(np.uint64)
        if not self.distinct:
            self.hist = np.zeros(1, dtype=np.uint64)

    def with_low(self, low_count: int) -> "Counts":
        """The same count kept from another low_count on (the reference's own build keeps every
        mer, whatever its -L: that is low_count 1)."""
        import copy
        c = copy.copy(self)
        c.low_count = low_count
        return c

    def frequent(self, min_count: int = 0):
        keep = self.all_counts >= max(min_count, self.low_count)
        return self.all_mers[keep].astype(np.uint64), self.all_counts[keep].astype(np.uint32)

    def info_text(self) -> bytes:
        return (f"Found {self.total} mers.\nFound {self.distinct} distinct mers.\n"
                f"Found {self.unique} unique mers.\nLargest mercount is {self.largest}.\n"
                ).encode()

    def histogram_text(self) -> bytes:
        rows, d, t = [], 0, 0
        for c in range(1, self.hist.shape[0]):
            h = int(self.hist[c])
            if h:
                d += h
                t += h * c
                rows.append("%d\t%d\t%.4f\t%.4f\n" % (c, h, d / self.distinct, t / self.total))
        return "".join(rows).encode()

    def threshold_text(self, min_count: int) -> bytes:
        mers, counts = self.frequent(min_count)
        out = []
        for m, c in zip(mers.tolist(), counts.tolist()):
            s = "".join("ACGT"[(m >> (2 * (self.k - 1 - i))) & 3] for i in range(self.k))
            out.append(f">{c}\n{s}\n")
        return "".join(out).encode()


def count_reads(rs, k: int, canonical: bool = True, low_count: int = 2) -> Counts:
    return Counts(all_mers(rs.bases, rs.offsets, rs.lengths, k, canonical), k, low_count)


# ------------------------------------------------------------------ fixtures and databases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["a_k16", "a_k5", "a_k31", "a_k32", "b_k22", "c_k16"]
_CACHE: dict = {}


def golden(name: str):
    """tests/golden/meryl_<name>.npz (tools/make_meryl_golden.py) as (reads, k, texts, numpy
    count); loaded and counted once per process, never modified."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"meryl_{name}.npz"))
        rs = types.SimpleNamespace(bases=z["bases"], offsets=z["offsets"], lengths=z["lengths"],
                                   quals=None, first_iid=1, nreads=int(z["lengths"].shape[0]))
        k = int(z["k"][0])
        texts = {"histogram": z["histogram"].tobytes(), "info": z["info"].tobytes(),
                 "dt": {int(t): z[f"dt_{int(t)}"].tobytes() for t in z["thresholds"]}}
        _CACHE[name] = (rs, k, texts, count_reads(rs, k))
    return _CACHE[name]


def write_db(prefix: str, c: Counts, canonical: bool = True) -> None:
    """prefix.mcidx / prefix.mcdat as canu_amd/csrc/meryl_host.h lays them out."""
    mers, counts = c.frequent(0)
    nz = np.nonzero(c.hist)[0]
    nz = nz[nz > 0]
    with open(prefix + ".mcidx", "wb") as f:
        f.write(b"CAMERIDX" + struct.pack("<IIII", 1, c.k, 1 if canonical else 0, c.low_count))
        f.write(struct.pack("<QQQQQQ", c.total, c.distinct, c.unique, c.largest,
                            mers.shape[0], nz.shape[0]))
        for n in nz.tolist():
            f.write(struct.pack("<QQ", n, int(c.hist[n])))
        f.write(b"XDIREMAC")
    with open(prefix + ".mcdat", "wb") as f:
        f.write(b"CAMERDAT" + struct.pack("<IIQ", 1, c.k, mers.shape[0]))
        f.write(mers.astype("<u8").tobytes() + counts.astype("<u4").tobytes() + b"TADREMAC")
