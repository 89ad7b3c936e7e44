"""canu's correctOverlaps (the second half of overlap error adjustment) over the MI355X C-ABI
(include/canu_co.h): src/overlapErrorAdjustment/correctOverlaps*.C.

`CorrectOverlaps.run` takes the overlaps of a read range as the overlap store holds them and the
`.red` records `FindErrors.run` gives, and returns the 12-bit evalue of each overlap on the
corrected reads -- the content of the `.oea` file that ovStoreBuild -evalues adds to the store.
`OverlapInCore.run -> store_view -> FindErrors.run -> CorrectOverlaps.run -> apply_evalues`
ends in the records bogart reads, with no file and no CPU aligner between the stages.  The
corrections and the alignments run in libcanu_co.so on a gfx950 device; there is no CPU
fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import struct

import numpy as np

from . import _capi
from ._capi import _atof, _atoi
from .find_errors import RED_DTYPE
from .overlap_in_core import RECORD_DTYPE

LIB_PATH = _capi.lib_path("co")

CO_STATUS = {0: "CO_OK", -1: "CO_ERR_NO_DEVICE", -2: "CO_ERR_BAD_PARAM",
             -3: "CO_ERR_UNSUPPORTED", -4: "CO_ERR_BAD_INPUT", -5: "CO_ERR_HIP",
             -6: "CO_ERR_OOM", -7: "CO_ERR_STATE"}

ABI_VERSION = 1                         # CO_ABI_VERSION of include/canu_co.h
WINDOW_DIAGS = 64                       # CO_WINDOW_DIAGS
LDS_BASES = 8192                        # CO_LDS_BASES
LOG_PER_ERROR = 128                     # CO_LOG_PER_ERROR

EVALUE_SHIFT = 42                       # ovOverlap.H:93-116: ahg5:21 ahg3:21 evalue:12
EVALUE_MASK = 0xFFF
AS_MAX_EVALUE = 4095                    # ovOverlap.H:41-42

# the nine counters Redo_Olaps prints, in its order (correctOverlaps-Redo_Olaps.C:543-552)
COUNTERS = ("olaps_fwd", "olaps_rev", "total", "failed_both", "failed_either", "failed_end",
            "failed_length", "rha_fail", "rha_pass")
# the numbers of Correct_Frags' "Corrected" line (correctOverlaps-Correct_Frags.C:327-331)
CORRECTED = ("corrected_bases", "substitutions", "deletions", "insertions")


class CoError(_capi.CapiError):
    STATUS = CO_STATUS


class _Params(ctypes.Structure):
    _fields_ = [("error_rate", ctypes.c_double)]


class _Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in COUNTERS + CORRECTED + (
        "rows", "bases", "regrows", "n_staged", "n_generic", "scratch_bytes")] + \
        [("ms_correct", ctypes.c_double), ("ms_align", ctypes.c_double)]


# Every symbol include/canu_co.h declares.
EXPORTS = ["co_params_init", "co_last_error", "co_abi_version", "co_ctx_create",
           "co_ctx_destroy", "co_set_params", "co_load_reads", "co_load_reads_device",
           "co_set_corrections", "co_correct_overlaps", "co_write_oea", "co_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_co.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_CO_LIB") or LIB_PATH
    lib = _capi.load("co", path, ABI_VERSION, CoError, _Params, _Stats)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.co_set_corrections.argtypes = [V, V, U64]
    lib.co_correct_overlaps.argtypes = [V, U32, U32, V, U64, V]
    lib.co_write_oea.argtypes = [V, ctypes.c_char_p]
    _lib = lib
    return lib


@dataclasses.dataclass
class CoParameters:
    """correctOverlaps' option that changes the result (correctOverlaps.H:271)."""
    error_rate: float = 0.06

    def to_c(self) -> _Params:
        return _Params(float(self.error_rate))


def parse_correctOverlaps_args(argv: list[str]) -> tuple[CoParameters, dict]:
    """correctOverlaps' command line (correctOverlaps.C:52-121) -> (parameters, the rest: gkp,
    ovl, red, out, bgn, end, threads, min_overlap).  -t and -l are parsed and change nothing, as
    there.  An unknown option or a missing -G / -O / -c / -o is an error, as there."""
    P = CoParameters()
    job = {"gkp": None, "ovl": None, "red": None, "out": None, "bgn": 0, "end": 0xFFFFFFFF,
           "threads": 1, "min_overlap": 0}
    i = 0

    def val(opt):
        nonlocal i
        if i + 1 >= len(argv):
            raise ValueError(f"correctOverlaps: option {opt} needs a value")
        i += 1
        return argv[i]

    while i < len(argv):
        a = argv[i]
        if a == "-G":
            job["gkp"] = val(a)
        elif a == "-O":
            job["ovl"] = val(a)
        elif a == "-c":
            job["red"] = val(a)
        elif a == "-o":
            job["out"] = val(a)
        elif a == "-R":
            job["bgn"] = _atoi(val(a)) & 0xFFFFFFFF
            job["end"] = _atoi(val(a)) & 0xFFFFFFFF
        elif a == "-e":
            P.error_rate = _atof(val(a))
        elif a == "-l":
            job["min_overlap"] = _atoi(val(a))
        elif a == "-t":
            job["threads"] = _atoi(val(a))
        else:
            raise ValueError(f"correctOverlaps: unknown option '{a}'")
        i += 1
    for k, opt in (("gkp", "-G"), ("ovl", "-O"), ("red", "-c"), ("out", "-o")):
        if job[k] is None:
            raise ValueError(f"correctOverlaps: no {opt} given")
    return P, job


def clamp_range(bgn: int, end: int, num_reads: int) -> tuple[int, int]:
    """correctOverlaps.C:146-150."""
    return (1 if bgn < 1 else bgn), (num_reads if num_reads < end else end)


class CorrectOverlaps(_capi.Context):
    """One correctOverlaps job on one gfx950 device: load reads, set the corrections, run ranges
    of overlaps."""
    PREFIX, ERROR, PARAMS, STATS = "co", CoError, CoParameters, _Stats

    def __init__(self, params: CoParameters | None = None, device: int = 0):
        super().__init__(load_library(), params, device)

    def set_corrections(self, red: np.ndarray) -> None:
        """The records of a .red file (RED_DTYPE, what FindErrors.run returns), ascending by
        read; every loaded read is corrected on the device."""
        rec = np.ascontiguousarray(red, dtype=RED_DTYPE)
        self._check(self.lib.co_set_corrections(self.ctx, rec.ctypes.data if rec.size else None,
                                                rec.shape[0]))

    def run(self, overlaps: np.ndarray, bgn_id: int, end_id: int) -> np.ndarray:
        """correctOverlaps -R bgn_id end_id over these overlaps -> uint16 evalues, one per
        overlap in input order."""
        rec = np.ascontiguousarray(overlaps, dtype=RECORD_DTYPE)
        out = np.zeros(rec.shape[0], dtype=np.uint16)
        self._check(self.lib.co_correct_overlaps(self.ctx, bgn_id, end_id,
                                                 rec.ctypes.data if rec.size else None,
                                                 rec.shape[0], out.ctypes.data if rec.size else None))
        return out

    def write_oea(self, path: str) -> None:
        self._check(self.lib.co_write_oea(self.ctx, os.fsencode(path)))

    def counters(self) -> dict:
        s = self.stats()
        return {n: s[n] for n in COUNTERS + CORRECTED}


def report(c: dict) -> str:
    """The lines correctOverlaps prints on stderr about its result: Correct_Frags' "Corrected"
    line (correctOverlaps-Correct_Frags.C:327-331) and Redo_Olaps' counters
    (correctOverlaps-Redo_Olaps.C:543-552)."""
    return (f"Corrected {c['corrected_bases']} bases with {c['substitutions']} substitutions, "
            f"{c['deletions']} deletions and {c['insertions']} insertions.\n"
            f"Olaps Fwd {c['olaps_fwd']}\n"
            f"Olaps Rev {c['olaps_rev']}\n"
            f"Total:  {c['total']}\n"
            f"Failed: {c['failed_both']} (both)\n"
            f"Failed: {c['failed_either']} (either)\n"
            f"Failed: {c['failed_end']} (match to end)\n"
            f"Failed: {c['failed_length']} (negative length)\n"
            f"rhaFail {c['rha_fail']} rhaPass {c['rha_pass']}\n")


def oea_bytes(bgn_id: int, end_id: int, evalues: np.ndarray) -> bytes:
    """The .oea file (correctOverlaps.C:203-215): int32 bgnID, int32 endID, uint64 n,
    uint16 evalue[n]."""
    ev = np.ascontiguousarray(evalues, dtype="<u2")
    return struct.pack("<IIQ", bgn_id & 0xFFFFFFFF, end_id & 0xFFFFFFFF, ev.shape[0]) + ev.tobytes()


def write_oea(path: str, bgn_id: int, end_id: int, evalues: np.ndarray) -> None:
    with open(path, "wb") as f:
        f.write(oea_bytes(bgn_id, end_id, evalues))


def parse_oea(raw: bytes) -> tuple[int, int, np.ndarray]:
    if len(raw) < 16:
        raise ValueError(f"an .oea file of {len(raw)} bytes has no header")
    bgn, end, n = struct.unpack("<IIQ", raw[:16])
    if len(raw) != 16 + 2 * n:
        raise ValueError(f"an .oea file of {len(raw)} bytes does not hold its {n} evalues")
    return bgn, end, np.frombuffer(raw, dtype="<u2", offset=16, count=n).copy()


def read_oea(path: str) -> tuple[int, int, np.ndarray]:
    """-> (bgn_id, end_id, evalues)."""
    with open(path, "rb") as f:
        return parse_oea(f.read())


def evalues_of(records: np.ndarray) -> np.ndarray:
    """The evalue field of ovOverlap records."""
    w0 = np.ascontiguousarray(records, dtype=RECORD_DTYPE)["w0"]
    return ((w0 >> np.uint64(EVALUE_SHIFT)) & np.uint64(EVALUE_MASK)).astype(np.uint16)


def apply_evalues(records: np.ndarray, evalues: np.ndarray) -> np.ndarray:
    """The records with their evalue replaced: what the store holds once ovStoreBuild -evalues
    has added the .oea files, and what bogart reads."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE).copy()
    ev = np.asarray(evalues)
    if ev.shape != rec.shape:
        raise ValueError(f"{ev.shape[0] if ev.ndim else 1} evalues for {rec.shape[0]} overlaps")
    if ev.size and (int(ev.min()) < 0 or int(ev.max()) > AS_MAX_EVALUE):
        raise ValueError("an evalue beyond 12 bits")
    keep = ~(np.uint64(EVALUE_MASK) << np.uint64(EVALUE_SHIFT))
    rec["w0"] = (rec["w0"] & keep) | (ev.astype(np.uint64) << np.uint64(EVALUE_SHIFT))
    return rec
