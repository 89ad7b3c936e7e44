"""canu's overlapPair over the MI355X C-ABI (include/canu_pair.h): the exact realignment of
MHAP (or minimap) overlaps, src/overlapInCore/overlapPair.C.

`OverlapPair.realign` takes ovOverlap records (the layout `OverlapInCore` returns and
`write_ovb` writes; `canu_amd.mhap.to_overlaps` makes them from MHAP result records) and returns
them realigned, in the same order, as the reference's recomputeOverlaps leaves them.  The
alignments run in libcanu_pair.so on a gfx950 device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os

import numpy as np

from .overlap_in_core import RECORD_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libcanu_pair.so")

PAIR_STATUS = {0: "PAIR_OK", -1: "PAIR_ERR_NO_DEVICE", -2: "PAIR_ERR_BAD_PARAM",
               -3: "PAIR_ERR_UNSUPPORTED", -4: "PAIR_ERR_BAD_INPUT", -5: "PAIR_ERR_HIP",
               -6: "PAIR_ERR_OOM", -7: "PAIR_ERR_STATE"}

ABI_VERSION = 1                         # PAIR_ABI_VERSION of include/canu_pair.h
LDS_COLUMNS = 16384                     # PAIR_LDS_COLUMNS
STRIPE_ROWS = 4096                      # PAIR_STRIPE_ROWS


class PairError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{PAIR_STATUS.get(code, code)}: {msg}")
        self.code = code


class _Params(ctypes.Structure):
    _fields_ = [("max_erate", ctypes.c_double), ("min_overlap_length", ctypes.c_uint32),
                ("partial", ctypes.c_int32), ("invert", ctypes.c_int32)]


class _Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "n_skipped", "n_passed", "n_failed", "n_fail_ext_a", "n_fail_ext_b", "n_fail_ext",
        "n_partial", "n_dovetail", "n_ext5a", "n_ext3a", "n_ext5b", "n_ext3b", "dp_cells",
        "dp_passes", "dp_steps", "scratch_bytes")] + [("ms_kernel", ctypes.c_double)]


# Every symbol include/canu_pair.h declares.
EXPORTS = ["pair_params_init", "pair_last_error", "pair_abi_version", "pair_ctx_create",
           "pair_ctx_destroy", "pair_set_params", "pair_load_reads", "pair_load_reads_device",
           "pair_realign", "pair_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_pair.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_PAIR_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise PairError(-1, f"{path} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    if lib.pair_abi_version() != ABI_VERSION:
        raise PairError(-1, f"{path} has ABI {lib.pair_abi_version()}, this binding expects "
                            f"{ABI_VERSION}: rebuild with __graft_entry__.build()")
    P, V, U32, U64 = ctypes.POINTER, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.pair_params_init.argtypes = [P(_Params)]
    lib.pair_params_init.restype = None
    lib.pair_last_error.restype = ctypes.c_char_p
    lib.pair_ctx_create.argtypes = [P(_Params), ctypes.c_int, P(V)]
    lib.pair_ctx_destroy.argtypes = [V]
    lib.pair_ctx_destroy.restype = None
    lib.pair_set_params.argtypes = [V, P(_Params)]
    lib.pair_load_reads.argtypes = [V, U32, U32, V, V, V]
    lib.pair_load_reads_device.argtypes = [V, U32, U32, V, V, V]
    lib.pair_realign.argtypes = [V, V, U64, V]
    lib.pair_get_stats.argtypes = [V, P(_Stats)]
    _lib = lib
    return lib


@dataclasses.dataclass
class PairParameters:
    """overlapPair's options (overlapPair.C:680-729).  The reference's default -len 0 hands
    its aligner empty spans; this port asks for 1 or more."""
    max_erate: float = 0.12
    min_overlap_length: int = 1
    partial: bool = False
    invert: bool = False

    def to_c(self) -> _Params:
        return _Params(float(self.max_erate), int(self.min_overlap_length),
                       1 if self.partial else 0, 1 if self.invert else 0)


def parse_overlapPair_args(argv: list[str]) -> tuple[PairParameters, dict]:
    """overlapPair's command line (overlapPair.C:690-729) -> (parameters, the rest: gkp, ovl,
    out, bgn, end, threads, memory).  Numbers parse as atoi / atof do; an unknown option or a
    missing -G / -O / -o is an error, as there."""
    P = PairParameters(min_overlap_length=0)
    job = {"gkp": None, "ovl": None, "out": None, "bgn": 0, "end": 0xFFFFFFFF, "threads": 1,
           "memory": 4}
    takes = {"-G": "gkp", "-O": "ovl", "-o": "out", "-b": "bgn", "-e": "end", "-t": "threads",
             "-memory": "memory"}

    def atoi(s: str) -> int:
        import re
        m = re.match(r"\s*[+-]?\d+", s)
        return int(m.group(0)) if m else 0

    def atof(s: str) -> float:
        import re
        m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", s)
        return float(m.group(0)) if m else 0.0

    i = 0
    while i < len(argv):
        a = argv[i]
        if a in takes or a in ("-erate", "-len"):
            if i + 1 >= len(argv):
                raise ValueError(f"overlapPair: option {a} needs a value")
            v = argv[i + 1]
            i += 1
            if a in ("-G", "-O", "-o"):
                job[takes[a]] = v
            elif a == "-erate":
                P.max_erate = atof(v)
            elif a == "-len":
                P.min_overlap_length = atoi(v)
            else:
                job[takes[a]] = atoi(v)
        elif a == "-partial":
            P.partial = True
        elif a == "-invert":
            P.invert = True
        else:
            raise ValueError(f"overlapPair: unknown option '{a}'")
        i += 1
    for k, opt in (("gkp", "-G"), ("ovl", "-O"), ("out", "-o")):
        if job[k] is None:
            raise ValueError(f"overlapPair: no {opt} given")
    return P, job


class OverlapPair:
    """One overlapPair job on one gfx950 device: load reads, realign batches of overlaps."""

    def __init__(self, params: PairParameters | None = None, device: int = 0):
        self.lib = load_library()
        self.params = params or PairParameters()
        self.ctx = None
        ctx = ctypes.c_void_p()
        cp = self.params.to_c()
        self._check(self.lib.pair_ctx_create(ctypes.byref(cp), device, ctypes.byref(ctx)))
        self.ctx = ctx

    def _check(self, rc: int):
        if rc != 0:
            raise PairError(rc, self.lib.pair_last_error().decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.pair_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params: PairParameters) -> None:
        cp = params.to_c()
        self._check(self.lib.pair_set_params(self.ctx, ctypes.byref(cp)))
        self.params = params

    def load_reads(self, rs) -> None:
        bases = np.ascontiguousarray(rs.bases, dtype=np.uint8)
        offs = np.ascontiguousarray(rs.offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
        self._check(self.lib.pair_load_reads(self.ctx, rs.first_iid, rs.nreads,
                                             bases.ctypes.data, offs.ctypes.data,
                                             lens.ctypes.data))

    def load_reads_device(self, first_iid: int, d_bases: int, d_offsets: int,
                          lengths: np.ndarray) -> None:
        """Reads already in HBM (device pointers, e.g. the buffers another stage loaded)."""
        lens = np.ascontiguousarray(lengths, dtype=np.uint32)
        self._check(self.lib.pair_load_reads_device(self.ctx, first_iid, lens.shape[0],
                                                    d_bases, d_offsets, lens.ctypes.data))

    def realign(self, records: np.ndarray) -> np.ndarray:
        """recomputeOverlaps over the records, in their order."""
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        out = np.zeros(rec.shape[0], dtype=RECORD_DTYPE)
        self._check(self.lib.pair_realign(self.ctx, rec.ctypes.data if rec.size else None,
                                          rec.shape[0], out.ctypes.data if rec.size else None))
        return out

    def stats(self) -> dict:
        s = _Stats()
        self._check(self.lib.pair_get_stats(self.ctx, ctypes.byref(s)))
        return {n: getattr(s, n) for n, _ in _Stats._fields_}

    def counters(self) -> dict:
        """The counters under alignStats' names (overlapPair.C:158-175)."""
        s = self.stats()
        return {"nSkipped": s["n_skipped"], "nPassed": s["n_passed"], "nFailed": s["n_failed"],
                "nFailExtA": s["n_fail_ext_a"], "nFailExtB": s["n_fail_ext_b"],
                "nFailExt": s["n_fail_ext"], "nPartial": s["n_partial"],
                "nDovetail": s["n_dovetail"], "nExt5a": s["n_ext5a"], "nExt3a": s["n_ext3a"],
                "nExt5b": s["n_ext5b"], "nExt3b": s["n_ext3b"]}


def report_final(c: dict) -> str:
    """alignStats::reportFinal's text (overlapPair.C:138-153) from `OverlapPair.counters()`."""
    tot = c["nPassed"] + c["nFailed"]
    if tot:
        pct = "%.4f" % (100.0 * c["nPassed"] / tot)
    else:
        pct = "-nan"
    return ("\n"
            f" -- {tot} overlaps processed.\n"
            f" -- {c['nSkipped']} skipped.\n"
            f" -- {c['nFailed']} failed {c['nPassed']} passed ({pct}%).\n"
            " --\n"
            f" -- {c['nFailExtA']} failed initial alignment, allowing A to extend\n"
            f" -- {c['nFailExtB']} failed initial alignment, allowing B to extend\n"
            f" -- {c['nFailExt']} failed initial alignment\n"
            " --\n"
            f" -- {c['nPartial']} partial overlaps (of any quality)\n"
            f" -- {c['nDovetail']} dovetail overlaps (before extensions, of any quality)\n"
            " --\n"
            f" -- {c['nExt5a']}/{c['nExt3a']} A read dovetail extensions\n"
            f" -- {c['nExt5b']}/{c['nExt3b']} B read dovetail extensions\n")
