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

from . import _capi
from ._capi import _atof, _atoi
from .overlap_in_core import RECORD_DTYPE

LIB_PATH = _capi.lib_path("pair")

PAIR_STATUS = {0: "PAIR_OK", -1: "PAIR_ERR_NO_DEVICE", -2: "PAIR_ERR_BAD_PARAM",
               -3: "PAIR_ERR_UNSUPPORTED", -4: "PAIR_ERR_BAD_INPUT", -5: "PAIR_ERR_HIP",
               -6: "PAIR_ERR_OOM", -7: "PAIR_ERR_STATE"}

ABI_VERSION = 1                         # PAIR_ABI_VERSION of include/canu_pair.h
LDS_COLUMNS = 16384                     # PAIR_LDS_COLUMNS
STRIPE_ROWS = 4096                      # PAIR_STRIPE_ROWS


class PairError(_capi.CapiError):
    STATUS = PAIR_STATUS


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
    lib = _capi.load("pair", path, ABI_VERSION, PairError, _Params, _Stats)
    lib.pair_realign.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
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
                P.max_erate = _atof(v)
            elif a == "-len":
                P.min_overlap_length = _atoi(v)
            else:
                job[takes[a]] = _atoi(v)
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


class OverlapPair(_capi.Context):
    """One overlapPair job on one gfx950 device: load reads, realign batches of overlaps."""
    PREFIX, ERROR, PARAMS, STATS = "pair", PairError, PairParameters, _Stats

    def __init__(self, params: PairParameters | None = None, device: int = 0):
        super().__init__(load_library(), params, device)

    def realign(self, records: np.ndarray) -> np.ndarray:
        """recomputeOverlaps over the records, in their order."""
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        out = np.zeros(rec.shape[0], dtype=RECORD_DTYPE)
        self._check(self.lib.pair_realign(self.ctx, rec.ctypes.data if rec.size else None,
                                          rec.shape[0], out.ctypes.data if rec.size else None))
        return out

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
