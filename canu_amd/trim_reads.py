"""canu's trimReads (overlap based trimming) over the MI355X C-ABI (include/canu_tr.h):
src/overlapBasedTrimming/trimReads*.C.

`TrimReads.run` takes the read lengths and the overlaps as an overlap store streams them (every
overlap of read a, sorted by a_iid: what `find_errors.store_view` gives) and returns each read's
clear range, its class (NOV / DEL / NOC / MOD) and the nine counters of the reference's .stats
file.  `OverlapInCore.run -> store_view -> TrimReads.run` needs no file in between; the
`TrimResult` writes the reference's three files (.clear, .log, .stats) byte for byte.  The trimming
runs in libcanu_tr.so on a gfx950 device; there is no CPU fallback.
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

LIB_PATH = _capi.lib_path("tr")

TR_STATUS = {0: "TR_OK", -1: "TR_ERR_NO_DEVICE", -2: "TR_ERR_BAD_PARAM", -3: "TR_ERR_UNSUPPORTED",
             -4: "TR_ERR_BAD_INPUT", -5: "TR_ERR_HIP", -6: "TR_ERR_OOM", -7: "TR_ERR_STATE"}

ABI_VERSION = 1                         # TR_ABI_VERSION of include/canu_tr.h
NOT_IN_RANGE, NOV, DEL, NOC, MOD = 0, 1, 2, 3, 4
TAGS = {NOV: "NOV", DEL: "DEL", NOC: "NOC", MOD: "MOD"}
FLAG_NO_HQ, FLAG_RESET = 1, 2
AS_MAX_EVALUE = 4095
U32_MAX = 0xFFFFFFFF

# the nine trimStat of trimReads.C:130-140
COUNTERS = ("reads_in", "deleted_in", "no_trim_in", "reads_out", "no_ovl_out", "deleted_out",
            "no_change_out", "trim5", "trim3")
LOG_HEADER = "id\tinitL\tinitR\tfinalL\tfinalR\tmessage (DEL=deleted NOC=no change MOD=modified)\n"


class TrError(_capi.CapiError):
    STATUS = TR_STATUS


class _Params(ctypes.Structure):
    _fields_ = [("erate", ctypes.c_double), ("min_read_length", ctypes.c_uint32),
                ("min_evidence_overlap", ctypes.c_uint32), ("min_evidence_coverage", ctypes.c_uint32)]


class _Count(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_uint64), ("bases", ctypes.c_uint64)]


class _Stats(ctypes.Structure):
    _fields_ = [(n, _Count) for n in COUNTERS] + \
        [("id_min", ctypes.c_uint32), ("id_max", ctypes.c_uint32)] + \
        [(n, ctypes.c_uint64) for n in ("n_overlaps", "n_wave_reads", "n_large_reads", "n_literal",
                                        "scratch_bytes")] + \
        [(n, ctypes.c_double) for n in ("ms_segment", "ms_wave", "ms_large")]


class _Result(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("bgn", "end", "status", "flags", "n_skipped", "n_used")]


# Every symbol include/canu_tr.h declares.
EXPORTS = ["tr_params_init", "tr_last_error", "tr_abi_version", "tr_wave_capacity", "tr_ctx_create",
           "tr_ctx_destroy", "tr_set_params", "tr_trim_reads", "tr_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_tr.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_TR_LIB") or LIB_PATH
    lib = _capi.load("tr", path, ABI_VERSION, TrError, _Params, _Stats, reads=False)
    V, U32 = ctypes.c_void_p, ctypes.c_uint32
    lib.tr_wave_capacity.restype = U32
    lib.tr_trim_reads.argtypes = [V, U32, V, V, V, ctypes.c_uint64, ctypes.c_int, U32, U32,
                                  ctypes.POINTER(_Result)]
    _lib = lib
    return lib


def wave_capacity() -> int:
    """The overlaps of one read a wave handles in LDS; a read with more takes the second path."""
    return int(load_library().tr_wave_capacity())


def encode_evalue(q: float) -> int:
    """AS_OVS_encodeEvalue, ovOverlap.H:44-45."""
    return int(10000.0 * q + 0.5) if q < AS_MAX_EVALUE / 10000.0 else AS_MAX_EVALUE


@dataclasses.dataclass
class TrParameters:
    """trimReads' options that change the result (trimReads.C:112-126)."""
    erate: float = 0.015
    min_read_length: int = 64
    min_evidence_overlap: int = 40
    min_evidence_coverage: int = 1

    def to_c(self) -> _Params:
        return _Params(float(self.erate), self.min_read_length & U32_MAX,
                       self.min_evidence_overlap & U32_MAX, self.min_evidence_coverage & U32_MAX)


def _decode_range(s: str) -> tuple[int, int]:
    """AS_UTL_decodeRange: "a" or "a-b"."""
    lo, _, hi = s.partition("-")
    return _atoi(lo) & U32_MAX, (_atoi(hi) if hi else _atoi(lo)) & U32_MAX


def parse_trimReads_args(argv: list[str]) -> tuple[TrParameters, dict]:
    """trimReads' command line (trimReads.C:145-218) -> (parameters, the rest: gkp, ovl, clear,
    out, id_min, id_max).  -Ci, -Cm and -l are refused: canu never passes them, the reference
    calls them unsupported and can assert with them.  A missing -Co is an error (the reference
    dereferences NULL there)."""
    P = TrParameters()
    job = {"gkp": None, "ovl": None, "clear": None, "out": None, "id_min": 1, "id_max": U32_MAX}
    i = 0

    def val(opt):
        nonlocal i
        if i + 1 >= len(argv):
            raise ValueError(f"trimReads: option {opt} needs a value")
        i += 1
        return argv[i]

    while i < len(argv):
        a = argv[i]
        if a == "-G":
            job["gkp"] = val(a)
        elif a == "-O":
            job["ovl"] = val(a)
        elif a == "-Co":
            job["clear"] = val(a)
        elif a == "-o":
            job["out"] = val(a)
        elif a == "-e":
            P.erate = _atof(val(a))
        elif a == "-minlength":
            P.min_read_length = _atoi(val(a)) & U32_MAX
        elif a == "-ol":
            P.min_evidence_overlap = _atoi(val(a)) & U32_MAX
        elif a == "-oc":
            P.min_evidence_coverage = _atoi(val(a)) & U32_MAX
        elif a == "-t":
            job["id_min"], job["id_max"] = _decode_range(val(a))
        elif a in ("-Ci", "-Cm", "-l"):
            raise ValueError(f"trimReads: option {a} is not supported")
        else:
            raise ValueError(f"trimReads: unknown option '{a}'")
        i += 1
    for k, opt in (("gkp", "-G"), ("ovl", "-O"), ("clear", "-Co"), ("out", "-o")):
        if job[k] is None:
            raise ValueError(f"trimReads: no {opt} given")
    return P, job


def parse_clear(raw: bytes, num_reads: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """A clear range file -> (bgn, end), each numReads + 1 long."""
    if len(raw) < 4:
        raise ValueError(f"a clear range file of {len(raw)} bytes has no read count")
    (n,) = struct.unpack("<I", raw[:4])
    if num_reads is not None and n != num_reads:
        raise ValueError(f"a clear range file for {n} reads, the store has {num_reads}")
    if len(raw) != 4 + 8 * (n + 1):
        raise ValueError(f"a clear range file of {len(raw)} bytes does not hold its {n} reads")
    v = np.frombuffer(raw, dtype="<u4", offset=4)
    return v[:n + 1].copy(), v[n + 1:].copy()


@dataclasses.dataclass
class TrimResult:
    """What trimReads decided.  The arrays have one entry per read, entry i for read i + 1;
    bgn / end are the log's finalL / finalR (the values the rule left, also for a deleted read)."""
    params: TrParameters
    lengths: np.ndarray
    bgn: np.ndarray
    end: np.ndarray
    status: np.ndarray                  # NOT_IN_RANGE, NOV, DEL, NOC, MOD
    flags: np.ndarray                   # FLAG_NO_HQ, FLAG_RESET
    n_skipped: np.ndarray
    n_used: np.ndarray
    counters: dict                      # name -> (reads, bases)
    id_min: int
    id_max: int
    stats: dict

    @property
    def num_reads(self) -> int:
        return int(self.lengths.shape[0])

    def clear_ranges(self) -> tuple[np.ndarray, np.ndarray]:
        """bgn, end as the -Co file holds them from entry 1 on: 0 .. length for a read left
        alone, UINT32_MAX twice for a deleted one."""
        bgn = np.zeros(self.num_reads, dtype=np.uint32)
        end = self.lengths.astype(np.uint32)
        gone = (self.status == NOV) | (self.status == DEL)
        mod = self.status == MOD
        bgn[gone] = end[gone] = U32_MAX
        bgn[mod], end[mod] = self.bgn[mod], self.end[mod]
        return bgn, end

    def clear_bytes(self, existing: bytes | None = None) -> bytes:
        """clearRangeFile.H:87-99: uint32 numReads, bgn[numReads + 1], end[numReads + 1].  An
        existing file is loaded and reset, which keeps its entry 0."""
        b0 = e0 = 0
        if existing is not None:
            ob, oe = parse_clear(existing, self.num_reads)
            b0, e0 = int(ob[0]), int(oe[0])
        bgn, end = self.clear_ranges()
        return struct.pack("<I", self.num_reads) + struct.pack("<I", b0) + bgn.astype("<u4").tobytes() + \
            struct.pack("<I", e0) + end.astype("<u4").tobytes()

    def log_text(self) -> str:
        out = [LOG_HEADER]
        for i in range(self.id_min - 1, self.id_max):
            st = int(self.status[i])
            if st == NOV:
                msg = ""
            elif self.flags[i] & FLAG_NO_HQ:
                msg = "\tno high quality overlaps"
            else:
                msg = f"\tskipped {int(self.n_skipped[i])} overlaps; used {int(self.n_used[i])} overlaps"
            out.append(f"{i + 1}\t0\t{int(self.lengths[i])}\t{int(self.bgn[i])}\t{int(self.end[i])}\t"
                       f"{TAGS[st]}{msg}\n")
        return "".join(out)

    def stats_text(self) -> str:
        """trimReads.C:469-504."""
        P, c = self.params, self.counters

        def row(k, what):
            return "%6u reads %12u bases (%s)\n" % (c[k][0], c[k][1], what)

        return ("PARAMETERS:\n----------\n"
                "%7u    (reads trimmed below this many bases are deleted)\n" % P.min_read_length +
                "%7.4f    (use overlaps at or below this fraction error)\n"
                % (encode_evalue(P.erate) / 10000.0) +
                "%7u    (break region if overlap is less than this long, for 'largest covered' algorithm)\n"
                % P.min_evidence_overlap +
                "%7u    (break region if overlap coverage is less than this many read%s, for 'largest "
                "covered' algorithm)\n" % (P.min_evidence_coverage,
                                           "" if P.min_evidence_coverage == 1 else "s") +
                "\nINPUT READS:\n-----------\n" +
                row("reads_in", "reads processed") +
                row("deleted_in", "reads not processed, previously deleted") +
                row("no_trim_in", "reads not processed, in a library where trimming isn't allowed") +
                "\nOUTPUT READS:\n------------\n" +
                row("reads_out", "trimmed reads output") +
                row("no_change_out", "reads with no change, kept as is") +
                row("no_ovl_out", "reads with no overlaps, deleted") +
                row("deleted_out", "reads with short trimmed length, deleted") +
                "\nTRIMMING DETAILS:\n----------------\n" +
                row("trim5", "bases trimmed from the 5' end of a read") +
                row("trim3", "bases trimmed from the 3' end of a read"))

    def stderr_text(self) -> str:
        """The "Processing" line (trimReads.C:262-265) and bestEdge's "iid" lines (:396)."""
        out = [f"Processing from ID {self.id_min} to {self.id_max} out of {self.num_reads} reads.\n"]
        out += [f"iid = {i + 1}\n" for i in np.flatnonzero(self.flags & FLAG_RESET)]
        return "".join(out)

    def write_clear(self, path: str) -> None:
        existing = None
        if os.path.exists(path):
            with open(path, "rb") as f:
                existing = f.read()
        with open(path, "wb") as f:
            f.write(self.clear_bytes(existing))

    def write_log(self, path: str) -> None:
        with open(path, "w") as f:
            f.write(self.log_text())

    def write_stats(self, path: str) -> None:
        with open(path, "w") as f:
            f.write(self.stats_text())


class TrimReads(_capi.Context):
    """One trimReads job on one gfx950 device.  It has no reads to load."""
    PREFIX, ERROR, PARAMS, STATS = "tr", TrError, TrParameters, _Stats

    def __init__(self, params: TrParameters | None = None, device: int = 0):
        super().__init__(load_library(), params, device)

    def run(self, read_lengths, records, rules=1, id_range=None, device_records: int | None = None,
            n_device_records: int = 0) -> TrimResult:
        """trimReads over reads 1 .. len(read_lengths).  records: the store view (RECORD_DTYPE,
        sorted by a_iid), or, with device_records, a device pointer to n_device_records of them
        already in HBM.  rules: finalTrim of every read's library (1 largestCovered, 2 bestEdge),
        one number or one per read.  id_range: -t, inclusive."""
        lens = np.ascontiguousarray(read_lengths, dtype=np.uint32)
        n = lens.shape[0]
        rl = np.ascontiguousarray(np.broadcast_to(np.asarray(rules, dtype=np.uint8), (n,)))
        id_min, id_max = id_range if id_range is not None else (1, U32_MAX)
        out = {"bgn": np.zeros(n, np.uint32), "end": np.zeros(n, np.uint32),
               "status": np.zeros(n, np.uint8), "flags": np.zeros(n, np.uint8),
               "n_skipped": np.zeros(n, np.uint32), "n_used": np.zeros(n, np.uint32)}
        res = _Result(*[out[k].ctypes.data for k, _ in _Result._fields_])
        if device_records is not None:
            ptr, cnt, on_dev = device_records, n_device_records, 1
        else:
            rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
            ptr, cnt, on_dev = (rec.ctypes.data if rec.size else None), rec.shape[0], 0
        self._check(self.lib.tr_trim_reads(self.ctx, n, lens.ctypes.data, rl.ctypes.data, ptr, cnt,
                                           on_dev, id_min & U32_MAX, id_max & U32_MAX,
                                           ctypes.byref(res)))
        s = self._stats()
        counters = {k: (getattr(s, k).reads, getattr(s, k).bases) for k in COUNTERS}
        stats = {k: getattr(s, k) for k, t in _Stats._fields_ if t is not _Count}
        return TrimResult(params=dataclasses.replace(self.params), lengths=lens, counters=counters,
                          id_min=s.id_min, id_max=s.id_max, stats=stats, **out)


def synth_store_view(n_reads: int, seed: int = 11, mean_overlaps: float = 10.0, n_large: int = 3,
                     large_overlaps: int = 3000, with_input: bool = False):
    """The synthetic store of fixed seed bench_tr.py runs on: reads of 500 .. 3000 bases, a skewed
    (log-normal) number of overlapper records per read, a few reads beyond the wave's capacity, and
    the view of these records an overlap store holds (each record and its twin, find_errors.
    store_view's content, sorted by a_iid alone).  -> (lengths, records), with_input: and the overlapper records."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(500, 3000, n_reads).astype(np.uint32)
    cnt = np.minimum(rng.lognormal(np.log(mean_overlaps) - 0.5, 1.0, n_reads).astype(np.int64), 200)
    cnt[rng.choice(n_reads, min(n_large, n_reads), replace=False)] = large_overlaps
    a = np.repeat(np.arange(1, n_reads + 1, dtype=np.uint32), cnt)
    m = a.shape[0]
    b = rng.integers(1, n_reads + 1, m).astype(np.uint32)

    def hangs(ids):
        # most overlaps reach an end of the read, ragged by up to 40 bases; a fifth are interior
        ln = lens[ids - 1].astype(np.int64)
        span = (ln * rng.uniform(0.2, 0.9, m)).astype(np.int64).clip(90)
        kind = rng.random(m)
        h5 = np.where(kind < 0.4, 0, np.where(kind < 0.8, ln - span, (rng.random(m) * (ln - span)).astype(np.int64)))
        h3 = ln - span - h5
        h5 = h5 + np.where((h5 == 0) & (rng.random(m) < 0.3), rng.integers(0, 40, m), 0)
        h3 = h3 + np.where((h3 == 0) & (rng.random(m) < 0.3), rng.integers(0, 40, m), 0)
        return h5.astype(np.uint64), h3.astype(np.uint64)

    a5, a3 = hangs(a)
    b5, b3 = hangs(b)
    ev = np.where(rng.random(m) < 0.03, 400, rng.integers(0, 150, m)).astype(np.uint64)
    s21, keep = np.uint64(21), (ev << np.uint64(42)) | (np.uint64(4) << np.uint64(55))   # forUTG
    both = np.zeros(2 * m, dtype=RECORD_DTYPE)
    both["a"][:m], both["b"][:m] = a, b
    both["w0"][:m], both["w1"][:m] = a5 | (a3 << s21) | keep, b5 | (b3 << s21)
    both["a"][m:], both["b"][m:] = b, a                 # the twin (ovOverlap.C:114), not flipped
    both["w0"][m:], both["w1"][m:] = b5 | (b3 << s21) | keep, a5 | (a3 << s21)
    view = both[np.argsort(both["a"], kind="stable")]
    return (lens, view, both[:m].copy()) if with_input else (lens, view)
