"""canu's falconsense (the consensus step of read correction) over the MI355X C-ABI
(include/canu_fs.h): src/correction/falconsense.C, falconConsensus*.C.

`FalconSense.run` takes correction layouts -- a template read and its evidence reads, as the
corStore holds them -- and returns the consensus of every template with its lower case;
`fasta_bytes` is what the program writes to stdout.  The alignments, the paths and the
consensus run in libcanu_fs.so on a gfx950 device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import re

import numpy as np

from . import _capi

LIB_PATH = _capi.lib_path("fs")

FS_STATUS = {0: "FS_OK", -1: "FS_ERR_NO_DEVICE", -2: "FS_ERR_BAD_PARAM",
             -3: "FS_ERR_UNSUPPORTED", -4: "FS_ERR_BAD_INPUT", -5: "FS_ERR_HIP",
             -6: "FS_ERR_OOM", -7: "FS_ERR_STATE"}

ABI_VERSION = 1                         # FS_ABI_VERSION of include/canu_fs.h
MIN_EVIDENCE = 500                      # FS_MIN_EVIDENCE
MAX_CHILDREN = 65535                    # FS_MAX_CHILDREN
LEAF_BYTES = 1048576                    # FS_LEAF_BYTES

LAYOUT_DTYPE = np.dtype([("tig_id", "<u4"), ("first_child", "<u4"), ("n_children", "<u4")])
CHILD_DTYPE = np.dtype([("ident", "<u4"), ("reverse", "<u4"), ("min", "<i4"), ("max", "<i4"),
                        ("askip", "<i4"), ("bskip", "<i4")])

# per layout: evidence reads aligned, skipped (shorter than 500) and rejected, template included
COUNTERS = ("aligned", "skipped", "rejected")


class FsError(_capi.CapiError):
    STATUS = FS_STATUS


class _Params(ctypes.Structure):
    _fields_ = [("min_coverage", ctypes.c_uint32), ("min_identity", ctypes.c_double),
                ("min_output_length", ctypes.c_uint32), ("hbm_budget", ctypes.c_uint64)]


_STAT_U64 = ("n_layouts", "n_evidence", "n_aligned", "n_skipped", "n_rejected", "n_tags", "dp_cells",
             "n_leaves", "n_splits", "n_batches", "scratch_bytes")
_STAT_F64 = ("ms_locate", "ms_path", "ms_sort", "ms_consensus")


class _Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in _STAT_U64] + [(n, ctypes.c_double) for n in _STAT_F64]


# Every symbol include/canu_fs.h declares.
EXPORTS = ["fs_params_init", "fs_last_error", "fs_abi_version", "fs_ctx_create", "fs_ctx_destroy",
           "fs_set_params", "fs_load_reads", "fs_load_reads_device", "fs_consensus",
           "fs_result_size", "fs_fetch", "fs_write_fasta_file", "fs_write_fasta", "fs_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_fs.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_FS_LIB") or LIB_PATH
    lib = _capi.load("fs", path, ABI_VERSION, FsError, _Params, _Stats)
    V, U64 = ctypes.c_void_p, ctypes.c_uint64
    lib.fs_consensus.argtypes = [V, V, U64, V, U64]
    lib.fs_result_size.argtypes = [V, ctypes.POINTER(U64), ctypes.POINTER(U64)]
    lib.fs_fetch.argtypes = [V, V, V, V]
    lib.fs_write_fasta.argtypes = [V, ctypes.c_char_p]
    _lib = lib
    return lib


@dataclasses.dataclass
class FsParameters:
    """falconsense's -cc, -ci and -cl.  min_identity is a double here; the program parses -ci
    with atoi, so canu's 0.x is 0 there, and 0 is the default."""
    min_coverage: int = 4
    min_identity: float = 0.0
    min_output_length: int = 500
    hbm_budget: int = 0                 # bytes of device scratch per batch of layouts; 0: 4 GiB

    def to_c(self) -> _Params:
        return _Params(int(self.min_coverage), float(self.min_identity),
                       int(self.min_output_length), int(self.hbm_budget))


def pieces(cns: bytes, min_output_length: int) -> list:
    """The corrected reads of one consensus: strtok(seq, "acgt") and the strict length test."""
    return [p for p in re.split(rb"[acgt]+", cns) if len(p) > min_output_length]


def fasta_of(tig_id: int, cns: bytes, min_output_length: int) -> bytes:
    out = bytearray()
    for k, p in enumerate(pieces(cns, min_output_length)):
        out += b">read%d_%d\n" % (tig_id, k)
        out += b"".join(p[i:i + 60] + b"\n" for i in range(0, len(p), 60))
    return bytes(out)


class FalconSense(_capi.Context):
    """One falconsense job on one gfx950 device: load reads, run layouts."""
    PREFIX, ERROR, PARAMS, STATS = "fs", FsError, FsParameters, _Stats

    def __init__(self, params: FsParameters | None = None, device: int = 0):
        self._tigs = np.zeros(0, dtype=np.uint32)
        super().__init__(load_library(), params, device)

    def run(self, layouts: np.ndarray, children: np.ndarray) -> list:
        """layouts: records with tig_id, first_child, n_children; children: records with ident,
        reverse, min, max, askip, bskip (more fields are ignored).  -> the consensus of every
        layout, lower case included, as bytes."""
        lay = np.zeros(len(layouts), dtype=LAYOUT_DTYPE)
        kid = np.zeros(len(children), dtype=CHILD_DTYPE)
        for f in LAYOUT_DTYPE.names:
            lay[f] = layouts[f]
        for f in CHILD_DTYPE.names:
            kid[f] = children[f]
        self._check(self.lib.fs_consensus(self.ctx, lay.ctypes.data if lay.size else None,
                                          lay.shape[0], kid.ctypes.data if kid.size else None,
                                          kid.shape[0]))
        n, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.fs_result_size(self.ctx, ctypes.byref(n), ctypes.byref(nb)))
        bases = np.zeros(max(nb.value, 1), dtype=np.uint8)
        offs = np.zeros(n.value + 1, dtype=np.uint64)
        cnt = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
        self._check(self.lib.fs_fetch(self.ctx, bases.ctypes.data, offs.ctypes.data, cnt.ctypes.data))
        self._tigs = lay["tig_id"].copy()
        self._counts = cnt[:n.value]
        self._cns = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(n.value)]
        return self._cns

    def fasta_bytes(self) -> bytes:
        """What falconsense writes to stdout for the layouts of the last run."""
        return b"".join(fasta_of(int(t), c, self.params.min_output_length)
                        for t, c in zip(self._tigs, self._cns))

    def write_fasta(self, path: str) -> None:
        self._check(self.lib.fs_write_fasta(self.ctx, os.fsencode(path)))

    def counters(self) -> np.ndarray:
        """Per layout of the last run: evidence reads aligned, skipped, rejected."""
        return self._counts


def synth_layouts(n_templates: int, read_len: int = 4000, coverage: int = 12, err: float = 0.10,
                  seed: int = 11):
    """Synthetic correction layouts for the benchmark: one genome, reads of about read_len at
    `coverage`, each read the template of the reads that overlap it by 1,000 bases or more,
    placed where the genome puts them.  -> (reads as a list of bytes, IDs from 1; layouts with
    tig_id, layout_len, first_child, n_children; children)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    n_reads = n_templates
    glen = max(read_len * 2, n_reads * read_len // coverage)
    genome = acgt[rng.integers(0, 4, glen)]
    reads, where = [], []
    for _ in range(n_reads):
        L = int(rng.integers(read_len * 3 // 4, read_len * 5 // 4))
        s = int(rng.integers(0, glen - L + 1))
        seg = genome[s:s + L]
        u = rng.random(L)
        sub = u < err / 3
        out = seg.copy()
        out[sub] = acgt[(np.searchsorted(acgt, seg[sub]) + rng.integers(1, 4, int(sub.sum()))) % 4]
        keep = ~((u >= err / 3) & (u < 2 * err / 3))           # deletions
        ins = (u >= 2 * err / 3) & (u < err)
        rep = np.where(keep, 1 + ins.astype(np.int64), 0)
        r = np.repeat(out, rep)
        strand = int(rng.integers(0, 2))
        b = r.tobytes()
        reads.append(b.translate(comp)[::-1] if strand else b)
        where.append((s, s + L, strand))
    lay = np.zeros(n_templates, dtype=np.dtype(LAYOUT_DTYPE.descr[:1] + [("layout_len", "<u4")] +
                                               LAYOUT_DTYPE.descr[1:]))
    kids = []
    for t in range(n_templates):
        ts, te, tst = where[t]
        tlen = len(reads[t])
        first = len(kids)
        for b in range(n_reads):
            bs, be, bst = where[b]
            lo, hi = max(ts, bs), min(te, be)
            if b == t or hi - lo < 1000:
                continue
            # where the shared stretch falls on the template and on the child, by proportion
            f = tlen / (te - ts)
            a_lo, a_hi = int((lo - ts) * f), int((hi - ts) * f)
            if tst:
                a_lo, a_hi = tlen - a_hi, tlen - a_lo
            blen = len(reads[b])
            g = blen / (be - bs)
            b_lo, b_hi = int((lo - bs) * g), int((hi - bs) * g)
            if bst:
                b_lo, b_hi = blen - b_hi, blen - b_lo
            rev = int(tst != bst)
            askip, bskip = (b_lo, blen - b_hi) if not rev else (blen - b_hi, b_lo)
            kids.append((b + 1, rev, max(a_lo, 0), min(max(a_hi, a_lo + 1), tlen), askip, bskip))
        lay[t] = (t + 1, tlen, first, len(kids) - first)
    return reads, lay, np.array(kids, dtype=CHILD_DTYPE).reshape(-1)
