"""canu's 0-mercounts stage over the MI355X C-ABI (include/canu_meryl.h).

`MerCounter` is `meryl -B -C -L 2 -m K` plus its two dump modes; `estimate_threshold` is
estimate-mer-threshold (src/meryl/estimate-mer-threshold.C:52-320) restated with its 32-bit
arithmetic; the functions below it restate the Perl glue of src/pipelines/canu/Meryl.pm
(:575-716), so that a caller without canu's Perl gets the same two files -- or hands the
k-mers to `OverlapInCore.set_skip_kmers` / `Mhap.set_kmer_frequencies` with no file at all.
The count runs in libcanu_meryl.so on a gfx950 device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import gzip
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libcanu_meryl.so")

MER_STATUS = {0: "MER_OK", -1: "MER_ERR_NO_DEVICE", -2: "MER_ERR_BAD_PARAM",
              -3: "MER_ERR_UNSUPPORTED", -4: "MER_ERR_BAD_INPUT", -5: "MER_ERR_HIP",
              -6: "MER_ERR_OOM", -7: "MER_ERR_STATE", -8: "MER_ERR_IO"}

ABI_VERSION = 1                         # MER_ABI_VERSION of include/canu_meryl.h
FIXED_OVERHEAD_BYTES = 48 << 20         # MER_FIXED_OVERHEAD_BYTES
MIN_BUDGET_BYTES = 4096 * 24            # MER_MIN_BUDGET_BYTES


class MerError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{MER_STATUS.get(code, code)}: {msg}")
        self.code = code


class _Params(ctypes.Structure):
    _fields_ = [("kmer_len", ctypes.c_uint32), ("canonical", ctypes.c_int32),
                ("low_count", ctypes.c_uint32), ("hbm_budget_bytes", ctypes.c_uint64)]


class _Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "total_mers", "distinct_mers", "unique_mers", "largest_count", "kept_mers", "passes",
        "direct_keys", "plan_scans", "oversize_buckets", "peak_device_bytes",
        "packed_read_bytes", "budget_bytes", "overflow_counts")] + \
        [(n, ctypes.c_double) for n in ("ms_plan", "ms_partition", "ms_sort", "ms_total")]


# Every symbol include/canu_meryl.h declares (tests check the library exports them all).
EXPORTS = ["mer_params_init", "mer_last_error", "mer_abi_version", "mer_ctx_create",
           "mer_ctx_destroy", "mer_load_reads", "mer_load_reads_device", "mer_count",
           "mer_get_stats", "mer_set_histogram_limits", "mer_get_params", "mer_histogram",
           "mer_frequent", "mer_save", "mer_open", "mer_write_histogram",
           "mer_write_threshold"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_meryl.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_MERYL_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise MerError(-1, f"{path} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    if lib.mer_abi_version() != ABI_VERSION:
        raise MerError(-1, f"{path} has ABI {lib.mer_abi_version()}, this binding expects "
                           f"{ABI_VERSION}: rebuild with __graft_entry__.build()")
    P, V, U64 = ctypes.POINTER, ctypes.c_void_p, ctypes.c_uint64
    lib.mer_params_init.argtypes = [P(_Params)]
    lib.mer_last_error.restype = ctypes.c_char_p
    lib.mer_ctx_create.argtypes = [P(_Params), ctypes.c_int, P(V)]
    lib.mer_ctx_destroy.argtypes = [V]
    lib.mer_ctx_destroy.restype = None
    lib.mer_load_reads.argtypes = [V, ctypes.c_uint32, V, V, V]
    lib.mer_load_reads_device.argtypes = [V, ctypes.c_uint32, V, V, V]
    lib.mer_count.argtypes = [V]
    lib.mer_get_stats.argtypes = [V, P(_Stats)]
    lib.mer_set_histogram_limits.argtypes = [V, ctypes.c_uint32, ctypes.c_uint32]
    lib.mer_get_params.argtypes = [V, P(_Params)]
    lib.mer_histogram.argtypes = [V, V, U64, P(U64)]
    lib.mer_frequent.argtypes = [V, U64, V, V, U64, P(U64)]
    lib.mer_save.argtypes = [V, ctypes.c_char_p]
    lib.mer_open.argtypes = [ctypes.c_char_p, P(V)]
    lib.mer_write_histogram.argtypes = [V, ctypes.c_char_p, ctypes.c_char_p]
    lib.mer_write_threshold.argtypes = [V, U64, ctypes.c_char_p]
    _lib = lib
    return lib


class MerCounter:
    """One k-mer count on one gfx950 device (`MerCounter.open` needs none)."""

    def __init__(self, k: int, canonical: bool = True, low_count: int = 2, device: int = 0,
                 hbm_budget: int | None = None, _ctx=None):
        self.lib = load_library()
        self.k = int(k)
        if _ctx is not None:
            self.ctx = _ctx
            return
        p = _Params(int(k), 1 if canonical else 0, int(low_count), int(hbm_budget or 0))
        ctx = ctypes.c_void_p()
        self.ctx = None
        self._check(self.lib.mer_ctx_create(ctypes.byref(p), device, ctypes.byref(ctx)))
        self.ctx = ctx

    @classmethod
    def open(cls, prefix: str) -> "MerCounter":
        """Reopen prefix.mcdat / prefix.mcidx (host only)."""
        lib = load_library()
        ctx = ctypes.c_void_p()
        rc = lib.mer_open(os.fsencode(prefix), ctypes.byref(ctx))
        if rc != 0:
            raise MerError(rc, lib.mer_last_error().decode())
        self = cls(0, _ctx=ctx)
        p = _Params()
        self._check(lib.mer_get_params(ctx, ctypes.byref(p)))
        self.k = int(p.kmer_len)
        return self

    def _check(self, rc: int):
        if rc != 0:
            raise MerError(rc, self.lib.mer_last_error().decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mer_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_reads(self, rs) -> None:
        bases = np.ascontiguousarray(rs.bases, dtype=np.uint8)
        offs = np.ascontiguousarray(rs.offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
        self._check(self.lib.mer_load_reads(self.ctx, lens.shape[0], bases.ctypes.data,
                                            offs.ctypes.data, lens.ctypes.data))

    def load_reads_device(self, d_bases: int, d_offsets: int, lengths: np.ndarray) -> None:
        """Reads already in HBM (device pointers, e.g. from torch tensors)."""
        lens = np.ascontiguousarray(lengths, dtype=np.uint32)
        self._check(self.lib.mer_load_reads_device(self.ctx, lens.shape[0], d_bases, d_offsets,
                                                   lens.ctypes.data))

    def set_histogram_limits(self, dense_len: int, overflow_cap: int) -> None:
        """Shorter device histogram / overflow list (mer_set_histogram_limits): same result,
        more passes."""
        self._check(self.lib.mer_set_histogram_limits(self.ctx, dense_len, overflow_cap))

    def params(self) -> dict:
        """The parameters in force (of a reopened database: the ones it was counted with)."""
        p = _Params()
        self._check(self.lib.mer_get_params(self.ctx, ctypes.byref(p)))
        return {"kmer_len": p.kmer_len, "canonical": bool(p.canonical),
                "low_count": p.low_count, "hbm_budget_bytes": p.hbm_budget_bytes}

    def count(self) -> "MerCounter":
        self._check(self.lib.mer_count(self.ctx))
        return self

    def stats(self) -> dict:
        s = _Stats()
        self._check(self.lib.mer_get_stats(self.ctx, ctypes.byref(s)))
        return {n: getattr(s, n) for n, _ in _Stats._fields_}

    def histogram(self) -> np.ndarray:
        """hist[c] = distinct mers with count c, dense up to the largest count."""
        n = ctypes.c_uint64()
        self._check(self.lib.mer_histogram(self.ctx, None, 0, ctypes.byref(n)))
        h = np.zeros(n.value, dtype=np.uint64)
        self._check(self.lib.mer_histogram(self.ctx, h.ctypes.data, n.value, ctypes.byref(n)))
        return h

    def frequent(self, min_count: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(mers, counts) with count >= max(min_count, low_count), in the dump's order."""
        n = ctypes.c_uint64()
        self._check(self.lib.mer_frequent(self.ctx, int(min_count), None, None, 0,
                                          ctypes.byref(n)))
        mers = np.zeros(n.value, dtype=np.uint64)
        counts = np.zeros(n.value, dtype=np.uint32)
        self._check(self.lib.mer_frequent(self.ctx, int(min_count), mers.ctypes.data,
                                          counts.ctypes.data, n.value, ctypes.byref(n)))
        return mers, counts

    def save(self, prefix: str) -> None:
        self._check(self.lib.mer_save(self.ctx, os.fsencode(prefix)))

    def write_histogram(self, hist_path: str | None, info_path: str | None) -> None:
        self._check(self.lib.mer_write_histogram(
            self.ctx, None if hist_path is None else os.fsencode(hist_path),
            None if info_path is None else os.fsencode(info_path)))

    def write_threshold(self, min_count: int, path: str) -> None:
        self._check(self.lib.mer_write_threshold(self.ctx, int(min_count), os.fsencode(path)))


def mers_to_strings(mers: np.ndarray, k: int) -> list[str]:
    """2-bit values (A<C<G<T, first base most significant) as upper-case strings."""
    m = np.asarray(mers, dtype=np.uint64)
    if m.size == 0:
        return []
    sh = (2 * (k - 1 - np.arange(k, dtype=np.uint64))).astype(np.uint64)
    codes = ((m[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8)
    txt = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [row.tobytes().decode() for row in txt]


_RC = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s: str) -> str:
    return s[::-1].translate(_RC)


# ---------------------------------------------------------------- estimate-mer-threshold

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def load_histogram_text(text: str) -> list[int]:
    """loadHistogram(FILE*) of estimate-mer-threshold.C:95-139: hist[h] = c as uint32, the
    array one longer than the largest h (its histLen)."""
    hist: dict[int, int] = {}
    hist_len = 0
    for line in text.split("\n"):
        if not line:
            continue
        w = line.split()
        h = int(w[0]) & _M32
        c = (int(w[1]) if len(w) > 1 else 0) & _M32
        hist[h] = c
        hist_len = max(hist_len, h)
    out = [0] * (hist_len + 1)
    for h, c in hist.items():
        out[h] = c
    return out


def guess_coverage(hist: list[int]) -> int:
    """guessCoverage (:52-70)."""
    n = len(hist)
    i = 2
    while i < n and hist[i - 1] > hist[i]:
        i += 1
    ix = i - 1
    while i < n:
        if hist[ix] < hist[i]:
            ix = i
        i += 1
    return ix


def estimate_threshold(hist, coverage: float = 0, log: list | None = None) -> int:
    """estimate-mer-threshold -h FILE [-c COV] (:184-320).  `hist` is the histogram text, or
    hist[count] = distinct mers as loaded from it.  Every product `hist[kk] * kk` is taken in
    32 bits before it is widened, as the reference's uint32 operands do; `log` collects the
    lines the reference writes to stderr."""
    if isinstance(hist, (str, bytes)):
        hist = load_histogram_text(hist.decode() if isinstance(hist, bytes) else hist)
    hist = [int(x) & _M32 for x in hist]
    n = len(hist)
    if n < 2:
        hist = hist + [0] * (2 - n)     # the reference's array is 1M entries of zero here
    say = (lambda s: log.append(s)) if log is not None else (lambda s: None)
    n_unique = hist[1] if n > 1 else 0
    n_distinct = sum(hist[:n]) & _M64
    n_total = sum((hist[h] * h) & _M32 for h in range(n)) & _M64
    say("RAW MER COUNTS:")
    say(f"  distinct: {n_distinct:12d} (different kmer sequences)")
    say(f"  unique:   {n_unique:12d} (single-copy kmers)")
    say(f"  total:    {n_total:12d} (kmers in sequences)")
    say("")
    if coverage > 0:
        guessed = float(coverage)
    else:
        guessed = float(guess_coverage(hist[:n] if n >= 2 else hist))
        say(f"Guessed X coverage is {int(guessed)}")

    useful_distinct = (n_distinct - n_unique) & _M64
    useful_all = (n_total - n_unique) & _M64
    distinct = total = 0
    max_count = ext_count = 0

    def div(a, b):                      # C double division (x/0 = inf, 0/0 = nan)
        a, b = float(a), float(b)
        if b == 0.0:
            return float("nan") if a == 0.0 else float("inf")
        return a / b

    def pct(a, b):
        v = div(100.0 * a, b)
        return "-nan" if v != v else ("inf" if v == float("inf") else f"{v:.2f}")

    def h(i):                           # the reference's array is far longer than histLen
        return hist[i] if i < len(hist) else 0

    kk = 2
    while kk < n:
        distinct = (distinct + hist[kk]) & _M64
        total = (total + ((hist[kk] * kk) & _M32)) & _M64
        if div(distinct, useful_distinct) > 0.9975 or \
                (div(total, useful_all) > 0.6667 and kk > 50 * guessed):
            max_count = kk
            break
        kk += 1
    say(f"Set maxCount to {max_count} ({h(max_count)} kmers), which will cover "
        f"{pct(distinct, useful_distinct)}% of distinct mers and {pct(total, useful_all)}% "
        f"of all mers.")

    lo = 2 if max_count < 27 else max_count - 25
    hi = n if max_count + 26 > n else max_count + 26
    avg = tot = 0
    # the loop index is int32, the bound uint32: compared as unsigned
    ii = lo
    while ii < hi:
        p = (ii * h(ii)) & _M32
        avg = (avg + p) & _M64
        tot = (tot + p) & _M64
        ii += 1
    span = (hi - lo) & _M32
    if span == 0:
        raise ZeroDivisionError("estimate-mer-threshold: empty averaging window")
    avg //= span
    say(f"Average number of kmers between count {lo} and {hi} is {avg}")

    while hi < n:
        if tot == 0:
            break
        tot = (tot - ((lo * h(lo)) & _M32)) & _M64
        tot = (tot + ((hi * h(hi)) & _M32)) & _M64
        lo += 1
        hi += 1
    if tot > 0:
        limit = n
        say("No break in kmer coverage found.")
    else:
        limit = lo
        say(f"Found break in kmer coverage at {limit}")

    while kk < limit:
        if ((avg * 10) & _M64) < ((kk * h(kk)) & _M32):
            break
        if div(total, useful_all) >= 0.9 and kk > 50 * guessed:
            break
        distinct = (distinct + h(kk)) & _M64
        total = (total + ((h(kk) * kk) & _M32)) & _M64
        if h(kk) > 0:
            ext_count = kk
        kk += 1
    if ext_count > 0:
        max_count = ext_count
    say(f"Set maxCount to {max_count} ({h(max_count)} kmers), which will cover "
        f"{pct(distinct, useful_distinct)}% of distinct mers and {pct(total, useful_all)}% "
        f"of all mers.")
    return max_count


# ------------------------------------------------------------------------- Meryl.pm's glue

def ovl_threshold(est: int | str, scale: float = 1.0) -> int:
    """merThresh = int(estimate * scale) + 1 (Meryl.pm:580)."""
    return int(float(est) * scale) + 1


def threshold_from_fractions(hist_text: str, thresh: int = 0, distinct: float | None = None,
                             total: float | None = None) -> int:
    """The merDistinct / merTotal scan of the histogram rows (Meryl.pm:586-611)."""
    if distinct is None and total is None:
        return thresh
    for line in hist_text.split("\n"):
        w = line.split()
        if len(w) < 4:
            continue
        t, d, f = int(w[0]), float(w[2]), float(w[3])
        if thresh > 0 and thresh < t:
            break
        if distinct is not None and distinct <= d:
            thresh = thresh if (thresh > 0 and thresh < t) else t
            break
        if total is not None and total <= f:
            thresh = thresh if (thresh > 0 and thresh < t) else t
            break
    return thresh


def histogram_texts(counter: MerCounter) -> tuple[str, str]:
    """(rows, info) of `meryl -Dh`."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        hp, ip = os.path.join(d, "h"), os.path.join(d, "i")
        counter.write_histogram(hp, ip)
        with open(hp) as f, open(ip) as g:
            return f.read(), g.read()


def skip_kmers(counter: MerCounter, thresh: int) -> list[str]:
    """The k-mers of `meryl -Dt -n thresh`, in its order: what `OverlapInCore.set_skip_kmers`
    takes (and what read_skip_fasta returns for the file write_ovl_frequent_mers writes)."""
    mers, _ = counter.frequent(thresh)
    return mers_to_strings(mers, counter.k)


def write_ovl_frequent_mers(counter: MerCounter, thresh: int, path: str) -> None:
    """<asm>.ms<K>.frequentMers.fasta: `meryl -Dt -n thresh` (Meryl.pm:634)."""
    counter.write_threshold(thresh, path)


def _mhap_filter(counter: MerCounter, filter_threshold: float) -> tuple[int, int, int]:
    """(totalMers, minCount, totalToOutput) of Meryl.pm:660-693."""
    rows, info = histogram_texts(counter)
    total_mers = 0
    for line in info.split("\n"):
        m = re.search(r"Found\s+(\d+)\s+mers.", line)
        if m:
            total_mers = 2 * int(m.group(1))
    if total_mers == 0:
        raise MerError(-4, "didn't find any mers?")
    min_count = int(filter_threshold * total_mers)
    # Meryl.pm counts the lines from the histogram and takes them from the dump; the two agree
    # only when the database holds every mer from min_count on.  The reference's always does
    # (its build ignores -L); one counted here with a larger low_count does not, and would
    # give a first line that promises more k-mers than follow
    low = counter.params()["low_count"]
    if max(min_count, 1) < low:
        raise MerError(-2, f"the filter threshold gives minCount {min_count}, below the "
                           f"low_count {low} this database was counted with: its count-"
                           f"{max(min_count, 1)}..{low - 1} mers are not kept; count with "
                           f"low_count <= {max(min_count, 1)} (meryl -L) for so few mers")
    to_output = 0
    for line in rows.split("\n"):
        w = line.split()
        if len(w) >= 2 and int(w[0]) >= min_count:
            to_output += int(w[1])
    return total_mers, min_count, 2 * to_output


def mhap_frequencies(counter: MerCounter, filter_threshold: float = 0.000005
                     ) -> tuple[list[str], np.ndarray, int]:
    """(k-mers, fractions, count line) of the -f file (Meryl.pm:650-716), in file order: what
    `Mhap.set_kmer_frequencies(kmers, fractions, expected)` takes.  The fractions are the
    values the file's %e text parses back to, so both routes set the same doubles."""
    total_mers, min_count, to_output = _mhap_filter(counter, filter_threshold)
    mers, counts = counter.frequent(min_count)
    kmers, fr = [], []
    for s, c in zip(mers_to_strings(mers, counter.k), counts.tolist()):
        v = float("%e" % (c / total_mers))
        kmers += [s, revcomp(s)]
        fr += [v, v]
    return kmers, np.asarray(fr, dtype=np.float64), to_output


def write_mhap_ignore(counter: MerCounter, filter_threshold: float, path: str) -> None:
    """<asm>.ms<K>.frequentMers.ignore.gz (Meryl.pm:650-716)."""
    total_mers, min_count, to_output = _mhap_filter(counter, filter_threshold)
    mers, counts = counter.frequent(min_count)
    with gzip.open(path, "wt") as f:
        f.write("%d\n" % to_output)
        for s, c in zip(mers_to_strings(mers, counter.k), counts.tolist()):
            f.write("%s\t%e\n" % (s, c / total_mers))
            f.write("%s\t%e\n" % (revcomp(s), c / total_mers))
