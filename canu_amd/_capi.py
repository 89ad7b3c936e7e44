"""What the ctypes bindings of find_errors, correct_overlaps, pair, falconsense, trim_reads and
split_reads share: the loader of a libcanu_*.so, the error and context base classes, and C's atoi / atof."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _atoi(s: str) -> int:
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group(0)) if m else 0


def _atof(s: str) -> float:
    m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", s)
    return float(m.group(0)) if m else 0.0


def lib_path(prefix: str) -> str:
    return os.path.join(HERE, "lib", f"libcanu_{prefix}.so")


class CapiError(RuntimeError):
    """"<STATUS NAME>: <message>" with the status in .code; a module's error names its STATUS."""
    STATUS: dict = {}

    def __init__(self, code: int, msg: str):
        super().__init__(f"{self.STATUS.get(code, code)}: {msg}")
        self.code = code


def load(prefix: str, path: str, abi: int, error, params, stats, reads: bool = True):
    """libcanu_<prefix>.so at `path` with the argtypes of the calls every library has; `reads`:
    and of <prefix>_load_reads[_device].  Raises `error` if it was not built or is of another ABI
    -- there is no fallback."""
    if not os.path.exists(path):
        raise error(-1, f"{path} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)

    def f(name):
        return getattr(lib, f"{prefix}_{name}")

    if f("abi_version")() != abi:
        raise error(-1, f"{path} has ABI {f('abi_version')()}, this binding expects "
                        f"{abi}: rebuild with __graft_entry__.build()")
    P, V, U32 = ctypes.POINTER, ctypes.c_void_p, ctypes.c_uint32
    f("params_init").argtypes = [P(params)]
    f("params_init").restype = None
    f("last_error").restype = ctypes.c_char_p
    f("ctx_create").argtypes = [P(params), ctypes.c_int, P(V)]
    f("ctx_destroy").argtypes = [V]
    f("ctx_destroy").restype = None
    f("set_params").argtypes = [V, P(params)]
    f("get_stats").argtypes = [V, P(stats)]
    if reads:
        f("load_reads").argtypes = [V, U32, U32, V, V, V]
        f("load_reads_device").argtypes = [V, U32, U32, V, V, V]
    return lib


class Context:
    """One job on one gfx950 device.  A subclass names its PREFIX, its ERROR, its parameters
    dataclass (PARAMS, with to_c) and its stats structure (STATS), and loads its library."""
    PREFIX = ""
    ERROR = CapiError
    PARAMS = None
    STATS = None

    def __init__(self, lib, params=None, device: int = 0):
        self.lib = lib
        self.params = params or self.PARAMS()
        self.ctx = None
        ctx = ctypes.c_void_p()
        cp = self.params.to_c()
        self._check(self._call("ctx_create")(ctypes.byref(cp), device, ctypes.byref(ctx)))
        self.ctx = ctx

    def _call(self, name: str):
        return getattr(self.lib, f"{self.PREFIX}_{name}")

    def _check(self, rc: int):
        if rc != 0:
            raise self.ERROR(rc, self._call("last_error")().decode())

    def close(self):
        if getattr(self, "ctx", None):
            self._call("ctx_destroy")(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params) -> None:
        cp = params.to_c()
        self._check(self._call("set_params")(self.ctx, ctypes.byref(cp)))
        self.params = params

    def load_reads(self, rs) -> None:
        bases = np.ascontiguousarray(rs.bases, dtype=np.uint8)
        offs = np.ascontiguousarray(rs.offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
        self._check(self._call("load_reads")(self.ctx, rs.first_iid, rs.nreads, bases.ctypes.data,
                                             offs.ctypes.data, lens.ctypes.data))

    def load_reads_device(self, first_iid: int, d_bases: int, d_offsets: int,
                          lengths: np.ndarray) -> None:
        """Reads already in HBM (device pointers, e.g. the buffers another stage loaded)."""
        lens = np.ascontiguousarray(lengths, dtype=np.uint32)
        self._check(self._call("load_reads_device")(self.ctx, first_iid, lens.shape[0], d_bases,
                                                    d_offsets, lens.ctypes.data))

    def _stats(self):
        s = self.STATS()
        self._check(self._call("get_stats")(self.ctx, ctypes.byref(s)))
        return s

    def stats(self) -> dict:
        s = self._stats()
        return {n: getattr(s, n) for n, _ in self.STATS._fields_}
