"""canu's splitReads (subread detection and read splitting, the second half of overlap based
trimming) over the MI355X C-ABI (include/canu_sr.h): src/overlapBasedTrimming/splitReads*.C.

`SplitReads.run` takes the read lengths, each read's library switches, the input clear ranges
(what trimReads left) and the overlaps as an overlap store streams them (sorted by (a_iid, b_iid):
what `find_errors.store_view` gives) and returns each read's final clear range, its class, the
confirmed bad regions and the counters of the reference's .stats file.
`OverlapInCore.run -> store_view -> TrimReads.run -> SplitReads.run(clear=trim_result)` needs no
file in between; the `SplitResult` writes the reference's three files (.clear, .log, .stats) byte
for byte.  The work runs in libcanu_sr.so on a gfx950 device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import struct

import numpy as np

from . import _capi
from ._capi import _atof, _atoi
from .find_errors import store_view  # noqa: F401  (the chain's middle)
from .overlap_in_core import RECORD_DTYPE
from .trim_reads import _decode_range, parse_clear

LIB_PATH = _capi.lib_path("sr")

SR_STATUS = {0: "SR_OK", -1: "SR_ERR_NO_DEVICE", -2: "SR_ERR_BAD_PARAM", -3: "SR_ERR_UNSUPPORTED",
             -4: "SR_ERR_BAD_INPUT", -5: "SR_ERR_HIP", -6: "SR_ERR_OOM", -7: "SR_ERR_STATE"}

ABI_VERSION = 1                         # SR_ABI_VERSION of include/canu_sr.h
LIB_ELIGIBLE, LIB_SUBREADS = 1, 2
RECORDS_ON_DEVICE, CLEAR_ON_DEVICE = 1, 2
NOT_IN_RANGE, DELETED_IN, NO_TRIM, NO_OVERLAPS, NO_COVERAGE, NO_CHANGE, TRIMMED, DELETED_OUT = range(8)
FATE_NOT_IN_RANGE, FATE_DROPPED, FATE_KEPT, FATE_MANY, FATE_SAME_ORIENT = range(5)
U32_MAX = 0xFFFFFFFF

# the trimStat of splitReads.C:64-114, in the order of sr_stats
COUNTERS = ("reads_in", "deleted_in", "no_trim_in", "no_overlaps", "no_coverage", "proc_chimera",
            "proc_spur", "proc_subread", "reads_bad_spur5", "reads_bad_spur3", "reads_bad_chimera",
            "reads_bad_subread", "bases_bad_spur5", "bases_bad_spur3", "bases_bad_chimera",
            "bases_bad_subread", "trimmed5", "trimmed3", "no_change", "deleted_out")

REGION_DTYPE = np.dtype([("read", "<u4"), ("bgn", "<u4"), ("end", "<u4")])


class SrError(_capi.CapiError):
    STATUS = SR_STATUS


class _Params(ctypes.Structure):
    _fields_ = [("erate", ctypes.c_double), ("min_read_length", ctypes.c_uint32)]


class _Count(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_uint64), ("bases", ctypes.c_uint64)]


class _Stats(ctypes.Structure):
    _fields_ = [(n, _Count) for n in COUNTERS] + \
        [("id_min", ctypes.c_uint32), ("id_max", ctypes.c_uint32)] + \
        [(n, ctypes.c_uint64) for n in ("n_overlaps", "n_wave_reads", "n_large_reads", "n_regions",
                                        "scratch_bytes")] + \
        [(n, ctypes.c_double) for n in ("ms_records", "ms_wave", "ms_large")]


class _Result(ctypes.Structure):
    _fields_ = [("bgn", ctypes.c_void_p), ("end", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("n_adjusted", ctypes.c_void_p), ("n_bad_regions", ctypes.c_void_p),
                ("fate", ctypes.c_void_p), ("regions", ctypes.c_void_p),
                ("regions_cap", ctypes.c_uint64), ("region_off", ctypes.c_void_p)]


# Every symbol include/canu_sr.h declares.
EXPORTS = ["sr_params_init", "sr_last_error", "sr_abi_version", "sr_wave_capacity", "sr_ctx_create",
           "sr_ctx_destroy", "sr_set_params", "sr_split_reads", "sr_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_sr.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_SR_LIB") or LIB_PATH
    lib = _capi.load("sr", path, ABI_VERSION, SrError, _Params, _Stats, reads=False)
    V, U32 = ctypes.c_void_p, ctypes.c_uint32
    lib.sr_wave_capacity.restype = U32
    lib.sr_split_reads.argtypes = [V, U32, V, V, V, V, V, ctypes.c_uint64, ctypes.c_int, U32, U32,
                                   ctypes.POINTER(_Result)]
    _lib = lib
    return lib


def wave_capacity() -> int:
    """The overlaps of one read a wave handles in LDS; a read with more takes the second path."""
    return int(load_library().sr_wave_capacity())


@dataclasses.dataclass
class SrParameters:
    """splitReads' options (splitReads.C:120-152)."""
    erate: float = 0.015
    min_read_length: int = 64

    def to_c(self) -> _Params:
        return _Params(float(self.erate), self.min_read_length & U32_MAX)


def parse_splitReads_args(argv: list[str]) -> tuple[SrParameters, dict]:
    """splitReads' command line (splitReads.C:120-152) -> (parameters, the rest: gkp, ovl,
    clear_in, clear, out, id_min, id_max).  A missing -Co is an error (the reference dereferences
    NULL there); a missing -Ci leaves clear_in None: every read starts at 0 .. length."""
    P = SrParameters()
    job = {"gkp": None, "ovl": None, "clear_in": None, "clear": None, "out": None, "id_min": 0,
           "id_max": U32_MAX}
    i = 0

    def val(opt):
        nonlocal i
        if i + 1 >= len(argv):
            raise ValueError(f"splitReads: option {opt} needs a value")
        i += 1
        return argv[i]

    while i < len(argv):
        a = argv[i]
        if a == "-G":
            job["gkp"] = val(a)
        elif a == "-O":
            job["ovl"] = val(a)
        elif a == "-Ci":
            job["clear_in"] = val(a)
        elif a == "-Co":
            job["clear"] = val(a)
        elif a == "-o":
            job["out"] = val(a)
        elif a == "-e":
            P.erate = _atof(val(a))
        elif a == "-minlength":
            P.min_read_length = _atoi(val(a)) & U32_MAX
        elif a == "-t":
            job["id_min"], job["id_max"] = _decode_range(val(a))
        else:
            raise ValueError(f"splitReads: unknown option '{a}'")
        i += 1
    if P.erate < 0.0:
        raise ValueError(f"splitReads: error rate (-e) value {P.erate:f} too small")
    for k, opt in (("gkp", "-G"), ("ovl", "-O"), ("clear", "-Co"), ("out", "-o")):
        if job[k] is None:
            raise ValueError(f"splitReads: no {opt} given")
    return P, job


@dataclasses.dataclass
class SplitResult:
    """What splitReads decided.  The per-read arrays have one entry per read, entry i for read
    i + 1; bgn / end are what trimBadInterval left (also for a read deleted on output), the input
    clear range where nothing was done."""
    params: SrParameters
    lengths: np.ndarray
    clear_in: tuple                     # (bgn, end) of every read on input
    bgn: np.ndarray
    end: np.ndarray
    status: np.ndarray                  # NOT_IN_RANGE .. DELETED_OUT
    n_adjusted: np.ndarray
    n_bad_regions: np.ndarray
    fate: np.ndarray                    # one per input record, FATE_*
    regions: np.ndarray                 # REGION_DTYPE, in read order
    region_off: np.ndarray              # regions of read i + 1: region_off[i] .. region_off[i + 1]
    error_pairs: np.ndarray             # (fate, a_iid, b_iid) of the records the ERROR lines name
    counters: dict                      # name -> (reads, bases)
    id_min: int
    id_max: int
    stats: dict

    @property
    def num_reads(self) -> int:
        return int(self.lengths.shape[0])

    def clear_ranges(self) -> tuple[np.ndarray, np.ndarray]:
        """bgn, end as the -Co file holds them from entry 1 on: the input range, the trimmed one,
        or UINT32_MAX twice for a read deleted here (or before)."""
        bgn, end = self.clear_in[0].copy(), self.clear_in[1].copy()
        t = self.status == TRIMMED
        bgn[t], end[t] = self.bgn[t], self.end[t]
        d = self.status == DELETED_OUT
        bgn[d] = end[d] = U32_MAX
        return bgn, end

    def clear_bytes(self, existing: bytes | None = None, entry0=(0, 0)) -> bytes:
        """clearRangeFile.H:87-99: uint32 numReads, bgn[numReads + 1], end[numReads + 1].  An
        existing -Co file is loaded, reset and overwritten from -Ci (splitReads.C:188-195), so only
        its read count matters; entry 0 is the -Ci file's (entry0), 0, 0 without one."""
        if existing is not None:
            parse_clear(existing, self.num_reads)
        bgn, end = self.clear_ranges()
        return struct.pack("<I", self.num_reads) + struct.pack("<I", entry0[0]) + \
            bgn.astype("<u4").tobytes() + struct.pack("<I", entry0[1]) + end.astype("<u4").tobytes()

    def log_text(self) -> str:
        """The reference never opens its subread log, so its log message stays empty."""
        return ""

    def stats_text(self) -> str:
        """splitReads.C:409-445."""
        P, c = self.params, self.counters

        def row(k, what, unit="bases"):
            return "%6u reads %12u %s (%s)\n" % (c[k][0], c[k][1], unit, what)

        return ("PARAMETERS:\n----------\n"
                "%7u    (reads trimmed below this many bases are deleted)\n" % P.min_read_length +
                "%7.4f    (use overlaps at or below this fraction error)\n" % P.erate +
                "INPUT READS:\n-----------\n" +
                row("reads_in", "reads processed") +
                row("deleted_in", "reads not processed, previously deleted") +
                row("no_trim_in", "reads not processed, in a library where trimming isn't allowed") +
                "\nPROCESSED:\n--------\n" +
                row("no_overlaps", "no overlaps") +
                row("no_coverage", "no coverage after adjusting for trimming done already") +
                row("proc_chimera", "processed for chimera") +
                row("proc_spur", "processed for spur") +
                row("proc_subread", "processed for subreads") +
                "\nREADS WITH SIGNALS:\n------------------\n" +
                row("reads_bad_spur5", "number of 5' spur signal", "signals") +
                row("reads_bad_spur3", "number of 3' spur signal", "signals") +
                row("reads_bad_chimera", "number of chimera signal", "signals") +
                row("reads_bad_subread", "number of subread signal", "signals") +
                "\nSIGNALS:\n-------\n" +
                row("bases_bad_spur5", "size of 5' spur signal") +
                row("bases_bad_spur3", "size of 3' spur signal") +
                row("bases_bad_chimera", "size of chimera signal") +
                row("bases_bad_subread", "size of subread signal") +
                "\nTRIMMING:\n--------\n" +
                row("trimmed5", "trimmed from the 5' end of the read") +
                row("trimmed3", "trimmed from the 3' end of the read"))

    def stderr_text(self) -> str:
        """The "Processing" line (splitReads.C:226-230) and detectSubReads' ERROR lines, in read
        and overlap order."""
        out = ["Processing from ID %u to %u out of %u reads, using errorRate = %.2f\n"
               % (self.id_min, self.id_max, self.num_reads, self.params.erate)]
        for f, a, b in self.error_pairs:
            out.append(f"ERROR: more overlaps than expected for pair {a} {b}.\n" if f == FATE_MANY
                       else f"ERROR: same orient duplicate overlaps for pair {a} {b}\n")
        return "".join(out)

    def write_clear(self, path: str, entry0=(0, 0)) -> None:
        existing = None
        if os.path.exists(path):
            with open(path, "rb") as f:
                existing = f.read()
        with open(path, "wb") as f:
            f.write(self.clear_bytes(existing, entry0))

    def write_log(self, path: str) -> None:
        with open(path, "w") as f:
            f.write(self.log_text())

    def write_stats(self, path: str) -> None:
        with open(path, "w") as f:
            f.write(self.stats_text())


def _clear_arrays(clear, n: int):
    """run()'s `clear` -> (bgn, end) of n reads, or None."""
    if clear is None:
        return None
    if hasattr(clear, "clear_ranges"):                  # a TrimResult, or a SplitResult
        clear = clear.clear_ranges()
    elif isinstance(clear, (bytes, bytearray, memoryview)):
        b, e = parse_clear(bytes(clear), n)
        clear = (b[1:], e[1:])
    b = np.ascontiguousarray(clear[0], dtype=np.uint32)
    e = np.ascontiguousarray(clear[1], dtype=np.uint32)
    if b.shape != (n,) or e.shape != (n,):
        raise ValueError(f"clear ranges of {b.shape[0]} and {e.shape[0]} reads for {n} reads")
    return b, e


class SplitReads(_capi.Context):
    """One splitReads job on one gfx950 device.  It has no reads to load."""
    PREFIX, ERROR, PARAMS, STATS = "sr", SrError, SrParameters, _Stats

    def __init__(self, params: SrParameters | None = None, device: int = 0):
        super().__init__(load_library(), params, device)

    def run(self, read_lengths, records, lib_flags=3, clear=None, id_range=None,
            device_records: int | None = None, n_device_records: int = 0,
            device_clear: tuple | None = None) -> SplitResult:
        """splitReads over reads 1 .. len(read_lengths).  records: the store view (RECORD_DTYPE,
        sorted by (a_iid, b_iid)); with device_records, a device pointer to n_device_records of
        them already in HBM, `records` then being their host copy or None (the ERROR lines of
        stderr_text need the host copy).  lib_flags: LIB_ELIGIBLE | LIB_SUBREADS of every read's
        library, one number or one per read.  clear: the input clear ranges -- a TrimResult, a
        (bgn, end) pair, or the bytes of a clear range file; device_clear: two device pointers to
        them instead.  id_range: -t, inclusive."""
        lens = np.ascontiguousarray(read_lengths, dtype=np.uint32)
        n = lens.shape[0]
        lf = np.ascontiguousarray(np.broadcast_to(np.asarray(lib_flags, dtype=np.uint8), (n,)))
        id_min, id_max = id_range if id_range is not None else (0, U32_MAX)
        rec = None if records is None else np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        on_dev = 0
        if device_records is not None:
            ptr, cnt, on_dev = device_records, n_device_records, RECORDS_ON_DEVICE
        else:
            ptr, cnt = (rec.ctypes.data if rec.size else None), rec.shape[0]
        if device_clear is not None:
            cb_ptr, ce_ptr = device_clear
            on_dev |= CLEAR_ON_DEVICE
            clr = None
        else:
            clr = _clear_arrays(clear, n)
            cb_ptr, ce_ptr = (clr[0].ctypes.data, clr[1].ctypes.data) if clr is not None and n else (None, None)
        out = {"bgn": np.zeros(n, np.uint32), "end": np.zeros(n, np.uint32),
               "status": np.zeros(n, np.uint8), "n_adjusted": np.zeros(n, np.uint32),
               "n_bad_regions": np.zeros(n, np.uint32), "fate": np.zeros(cnt, np.uint8)}
        regions = np.zeros(cnt // 2 + 1, dtype=REGION_DTYPE)
        region_off = np.zeros(n + 1, np.uint64)
        res = _Result(out["bgn"].ctypes.data, out["end"].ctypes.data, out["status"].ctypes.data,
                      out["n_adjusted"].ctypes.data, out["n_bad_regions"].ctypes.data,
                      out["fate"].ctypes.data, regions.ctypes.data, regions.shape[0],
                      region_off.ctypes.data)
        self._check(self.lib.sr_split_reads(self.ctx, n, lens.ctypes.data, lf.ctypes.data, cb_ptr, ce_ptr,
                                            ptr, cnt, on_dev, id_min & U32_MAX, id_max & U32_MAX,
                                            ctypes.byref(res)))
        s = self._stats()
        counters = {k: (getattr(s, k).reads, getattr(s, k).bases) for k in COUNTERS}
        stats = {k: getattr(s, k) for k, t in _Stats._fields_ if t is not _Count}
        if clr is not None:
            clear_in = clr
        elif device_clear is None:
            clear_in = (np.zeros(n, np.uint32), lens.copy())
        else:
            # the input ranges stayed on the device: bgn / end still hold them for every read the
            # library did not trim, which is all clear_ranges() needs
            kept = (out["status"] != TRIMMED) & (out["status"] != DELETED_OUT)
            clear_in = (np.where(kept, out["bgn"], 0).astype(np.uint32),
                        np.where(kept, out["end"], 0).astype(np.uint32))
        bad = np.flatnonzero(out["fate"] >= FATE_MANY)
        if rec is not None and rec.shape[0] == cnt:
            errs = np.stack([out["fate"][bad].astype(np.int64), rec["a"][bad].astype(np.int64),
                             rec["b"][bad].astype(np.int64)], axis=1) if bad.size else np.zeros((0, 3), np.int64)
        else:
            errs = np.zeros((0, 3), np.int64)
        return SplitResult(params=dataclasses.replace(self.params), lengths=lens, clear_in=clear_in,
                           regions=regions[:int(region_off[n])].copy(), region_off=region_off,
                           error_pairs=errs, counters=counters, id_min=s.id_min, id_max=s.id_max,
                           stats=stats, **out)


def synth_store_view(n_reads: int, seed: int = 13, mean_overlaps: float = 10.0, n_large: int = 3,
                     large_overlaps: int = 3000, junction_rate: float = 0.05, with_input: bool = False):
    """The synthetic store of fixed seed bench_sr.py runs on: trim_reads.synth_store_view's reads
    and overlapper records, and on a fraction of the reads a planted subread junction -- four to
    eight twin pairs (a forward and a flipped overlap with one B read each) that end and begin
    around one place of the A read, 0 .. 500 bases apart, and cover one stretch of the B read.
    The view is what an overlap store built from the records holds (find_errors.store_view: every
    record and its twin, sorted by a_iid, b_iid and the data words).
    -> (lengths, view), with_input: and the overlapper records."""
    from .trim_reads import synth_store_view as tr_view
    lens, _, recs = tr_view(n_reads, seed=seed, mean_overlaps=mean_overlaps, n_large=n_large,
                            large_overlaps=large_overlaps, with_input=True)
    rng = np.random.default_rng(seed + 1)
    flags = 4 << 55                                     # forUTG
    extra = []
    for a in np.flatnonzero(rng.random(n_reads) < junction_rate) + 1:
        la = int(lens[a - 1])
        if la < 1400:
            continue
        junction = int(rng.integers(450, la - 900))
        for _ in range(int(rng.integers(4, 9))):
            b = int(rng.integers(1, n_reads + 1))
            lb = int(lens[b - 1])
            gap = int(rng.integers(0, 501))
            span = min(int(rng.integers(300, 401)), lb)
            if b == a or junction + gap + span > la:
                continue
            b5 = int(rng.integers(0, lb - span + 1))
            w1 = b5 | ((lb - span - b5) << 21)
            extra.append((a, b, (junction - span) | ((la - junction) << 21) | flags, w1))
            extra.append((a, b, (junction + gap) | ((la - junction - gap - span) << 21) | (1 << 54) | flags, w1))
    if extra:
        recs = np.concatenate([recs, np.array(extra, dtype=RECORD_DTYPE)])
    view = store_view(recs)
    return (lens, view, recs) if with_input else (lens, view)
