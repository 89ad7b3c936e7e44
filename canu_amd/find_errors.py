"""canu's findErrors ("RED", the first half of overlap error adjustment) over the MI355X C-ABI
(include/canu_fe.h): src/overlapErrorAdjustment/findErrors*.C.

`FindErrors.run` takes the overlaps of a read range as the overlap store holds them (ovOverlap
records, the layout `OverlapInCore` returns; `store_view` makes a store's content from
overlapper output) and returns the records of the `.red` file.  The alignments, the votes and
the decisions run in libcanu_fe.so on a gfx950 device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os

import numpy as np

from . import _capi
from ._capi import _atof, _atoi  # noqa: F401  (other modules and tests take them from here)
from .overlap_in_core import RECORD_DTYPE

LIB_PATH = _capi.lib_path("fe")

FE_STATUS = {0: "FE_OK", -1: "FE_ERR_NO_DEVICE", -2: "FE_ERR_BAD_PARAM",
             -3: "FE_ERR_UNSUPPORTED", -4: "FE_ERR_BAD_INPUT", -5: "FE_ERR_HIP",
             -6: "FE_ERR_OOM", -7: "FE_ERR_STATE"}

ABI_VERSION = 1                         # FE_ABI_VERSION of include/canu_fe.h
WINDOW_DIAGS = 64                       # FE_WINDOW_DIAGS
LDS_BASES = 8192                        # FE_LDS_BASES
LOG_PER_ERROR = 128                     # FE_LOG_PER_ERROR

# Correction_Output_t (correctionOutput.H:40-46): word = keep_left | keep_right << 1 |
# type << 2 | pos << 6
RED_DTYPE = np.dtype([("word", "<u4"), ("readID", "<u4")])
VOTE_NAMES = ("IDENT", "DELETE", "A_SUBST", "C_SUBST", "G_SUBST", "T_SUBST", "A_INSERT",
              "C_INSERT", "G_INSERT", "T_INSERT", "NO_VOTE", "EXTENSION")


class FeError(_capi.CapiError):
    STATUS = FE_STATUS


class _Params(ctypes.Structure):
    _fields_ = [("error_rate", ctypes.c_double), ("degree_threshold", ctypes.c_int32),
                ("kmer_len", ctypes.c_int32), ("vote_qualify_len", ctypes.c_int32),
                ("end_exclude_len", ctypes.c_int32), ("use_haplo_ct", ctypes.c_int32)]


class _Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "n_passed", "n_failed", "n_generic", "n_staged", "rows", "bases", "regrows", "scratch_bytes")] + \
        [("ms_align", ctypes.c_double), ("ms_decide", ctypes.c_double)]


# Every symbol include/canu_fe.h declares.
EXPORTS = ["fe_params_init", "fe_last_error", "fe_abi_version", "fe_ctx_create",
           "fe_ctx_destroy", "fe_set_params", "fe_load_reads", "fe_load_reads_device",
           "fe_find_errors", "fe_fetch_corrections", "fe_write_red", "fe_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_fe.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_FE_LIB") or LIB_PATH
    lib = _capi.load("fe", path, ABI_VERSION, FeError, _Params, _Stats)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.fe_find_errors.argtypes = [V, U32, U32, V, U64, ctypes.POINTER(U64)]
    lib.fe_fetch_corrections.argtypes = [V, V, U64, ctypes.POINTER(U64)]
    lib.fe_write_red.argtypes = [V, ctypes.c_char_p]
    _lib = lib
    return lib


@dataclasses.dataclass
class FeParameters:
    """findErrors' options with the reference's defaults (findErrors.H:304-337)."""
    error_rate: float = 0.06
    degree_threshold: int = 2
    kmer_len: int = 9
    vote_qualify_len: int = 9
    end_exclude_len: int = 3
    use_haplo_ct: bool = True

    def to_c(self) -> _Params:
        return _Params(float(self.error_rate), int(self.degree_threshold), int(self.kmer_len),
                       int(self.vote_qualify_len), int(self.end_exclude_len),
                       1 if self.use_haplo_ct else 0)


def parse_findErrors_args(argv: list[str]) -> tuple[FeParameters, dict]:
    """findErrors' command line (findErrors.C:381-433) -> (parameters, the rest: gkp, ovl, out,
    bgn, end, threads, min_overlap).  -t and -l are parsed and change nothing, as there.  An
    unknown option or a missing -G / -O is an error, as there."""
    P = FeParameters()
    job = {"gkp": None, "ovl": None, "out": None, "bgn": 0, "end": 0xFFFFFFFF, "threads": 4,
           "min_overlap": 0}
    i = 0

    def val(opt):
        nonlocal i
        if i + 1 >= len(argv):
            raise ValueError(f"findErrors: option {opt} needs a value")
        i += 1
        return argv[i]

    while i < len(argv):
        a = argv[i]
        if a == "-G":
            job["gkp"] = val(a)
        elif a == "-O":
            job["ovl"] = val(a)
        elif a == "-o":
            job["out"] = val(a)
        elif a == "-R":
            job["bgn"] = _atoi(val(a))
            job["end"] = _atoi(val(a))
        elif a == "-e":
            P.error_rate = _atof(val(a))
        elif a == "-l":
            job["min_overlap"] = _atoi(val(a))
        elif a == "-t":
            job["threads"] = _atoi(val(a))
        elif a == "-d":
            P.degree_threshold = _atoi(val(a))
        elif a == "-k":
            P.kmer_len = _atoi(val(a))
        elif a == "-p":
            P.use_haplo_ct = False
        elif a == "-V":
            P.vote_qualify_len = _atoi(val(a))
        elif a == "-x":
            P.end_exclude_len = _atoi(val(a))
        else:
            raise ValueError(f"findErrors: unknown option '{a}'")
        i += 1
    for k, opt in (("gkp", "-G"), ("ovl", "-O")):
        if job[k] is None:
            raise ValueError(f"findErrors: no {opt} given")
    if job["threads"] == 0:
        raise ValueError("findErrors: number of compute threads (-t) must be larger than zero")
    return P, job


class FindErrors(_capi.Context):
    """One findErrors job on one gfx950 device: load reads, run ranges of overlaps."""
    PREFIX, ERROR, PARAMS, STATS = "fe", FeError, FeParameters, _Stats

    def __init__(self, params: FeParameters | None = None, device: int = 0):
        super().__init__(load_library(), params, device)

    def run(self, overlaps: np.ndarray, bgn_id: int, end_id: int) -> np.ndarray:
        """findErrors -R bgn_id end_id over these overlaps -> the .red records (RED_DTYPE)."""
        rec = np.ascontiguousarray(overlaps, dtype=RECORD_DTYPE)
        n = ctypes.c_uint64()
        self._check(self.lib.fe_find_errors(self.ctx, bgn_id, end_id,
                                            rec.ctypes.data if rec.size else None, rec.shape[0],
                                            ctypes.byref(n)))
        out = np.zeros(n.value, dtype=RED_DTYPE)
        self._check(self.lib.fe_fetch_corrections(self.ctx, out.ctypes.data if n.value else None,
                                                  n.value, ctypes.byref(n)))
        return out

    def write_red(self, path: str) -> None:
        self._check(self.lib.fe_write_red(self.ctx, os.fsencode(path)))

    def counters(self) -> dict:
        s = self.stats()
        return {"passed": s["n_passed"], "failed": s["n_failed"]}


def report(c: dict) -> str:
    """The two lines findErrors prints on stderr (findErrors.C:504-505)."""
    p, f = c["passed"], c["failed"]
    pct = (lambda v: "%8.4f" % (100.0 * v / (p + f))) if p + f else (lambda v: "%8s" % "-nan")
    return (f"Passed overlaps = {p:10d} {pct(p)}%\n"
            f"Failed overlaps = {f:10d} {pct(f)}%\n")


def read_red(path: str) -> np.ndarray:
    return np.fromfile(path, dtype=RED_DTYPE)


def dump_red(records: np.ndarray) -> str:
    """The text findErrors-Dump prints for a .red file (findErrors-Dump.C:85-92)."""
    out = []
    for r in records:
        w = int(r["word"])
        out.append("%8u %12s %8u %c %c\n" % (int(r["readID"]), VOTE_NAMES[(w >> 2) & 15], w >> 6,
                                             "t" if w & 1 else "f", "t" if w & 2 else "f"))
    return "".join(out)


def store_view(records: np.ndarray) -> np.ndarray:
    """What an overlap store built from these overlapper records holds: each overlap and its
    swapIDs twin (ovOverlap.C:114), sorted by a_iid, b_iid and the data words (ovOverlap.H:327).
    Records with none of forUTG / forOBT / forDUP set never reach a store.  The flag edits of
    ovStoreFilter are not applied; findErrors reads the IDs, the hangs and `flipped` only."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    rec = rec[((rec["w0"] >> np.uint64(55)) & np.uint64(7)) != 0]
    HM = np.uint64((1 << 21) - 1)
    s21 = np.uint64(21)
    w0, w1 = rec["w0"], rec["w1"]
    a5, a3, b5, b3 = w0 & HM, (w0 >> s21) & HM, w1 & HM, (w1 >> s21) & HM
    fl = ((w0 >> np.uint64(54)) & np.uint64(1)).astype(bool)
    keep0 = w0 & ~(HM | (HM << s21))
    keep1 = w1 & ~(HM | (HM << s21))
    twin = np.zeros(rec.shape[0], dtype=RECORD_DTYPE)
    twin["a"], twin["b"] = rec["b"], rec["a"]
    twin["w0"] = keep0 | np.where(fl, b3, b5) | (np.where(fl, b5, b3) << s21)
    twin["w1"] = keep1 | np.where(fl, a3, a5) | (np.where(fl, a5, a3) << s21)
    both = np.concatenate([rec, twin])
    return both[np.lexsort((both["w1"], both["w0"], both["b"], both["a"]))]
