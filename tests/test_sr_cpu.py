"""splitReads without a GPU: the restatement (tests/sr_restate.py) against the reference's own files
(tests/golden/sr_*.npz), the closed forms the kernel computes against the literal interval list,
the Python writers, the argument parser, the ABI, and the host code of the drop-in executable
under the sanitizers (tests/sr_host_check.cpp)."""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import sr_restate as SR  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("a", "b", "c", "d")
REC = np.dtype([("a", "<u4"), ("b", "<u4"), ("w0", "<u8"), ("w1", "<u8")])


def load(name):
    from canu_amd.split_reads import parse_splitReads_args
    fx = np.load(os.path.join(GOLDEN, f"sr_{name}.npz"))
    args = fx["args"].tobytes().decode().split()
    TP, job = parse_splitReads_args(args + ["-G", "g", "-O", "o", "-Co", "c", "-o", "p"])
    e0 = (0, 0)
    if "clear_in_file" in fx.files:
        b, e = SR.parse_clear(fx["clear_in_file"].tobytes())
        e0 = (int(b[0]), int(e[0]))
    return fx, args, TP, SR.Params(TP.erate, TP.min_read_length), (job["id_min"], job["id_max"]), e0


def restate(fx, P, rng, **kw):
    return SR.split_reads(fx["lengths"], fx["records"], fx["lib_flags"], tuple(fx["clear_in"]), P, rng, **kw)


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(name, closed):
    fx, args, TP, P, rng, e0 = load(name)
    R = restate(fx, P, rng, closed=closed)
    assert SR.clear_bytes(R, e0) == fx["clear"].tobytes()
    assert SR.log_text(R).encode() == fx["log"].tobytes() == b""
    assert SR.stats_text(R, P).encode() == fx["stats"].tobytes()
    assert SR.stderr_text(R, P, fx["records"]).encode() == fx["stderr"].tobytes()


def test_fixtures_are_small_and_reach_the_required_branches():
    br = {}
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, f"sr_{name}.npz")) < 64 * 1024
        fx, args, TP, P, rng, e0 = load(name)
        restate(fx, P, rng, branches=br)
    assert not [b for b in SR.REQUIRED_BRANCHES if not br.get(b)]
    # the reference's own lines: a group of three and a same-orientation pair
    err = np.load(os.path.join(GOLDEN, "sr_a.npz"))["stderr"].tobytes()
    assert err.count(b"ERROR: more overlaps than expected") == 6      # once per member, both reads
    assert err.count(b"ERROR: same orient duplicate overlaps") == 2   # once per pair
    # one fixture deletes where the other trims to nothing
    a, b = (restate(*[load(n)[k] for k in (0, 3, 4)]) for n in ("a", "b"))
    gone = np.flatnonzero(a["status"] == SR.DELETED_OUT)
    assert gone.size >= 2 and (b["status"][gone] == SR.TRIMMED).all()
    assert ((b["end"][gone] - b["bgn"][gone]) < 64).all() and (b["end"][gone] == b["bgn"][gone]).any()
    # the input clear file of d is the one the reference trimReads wrote
    d = np.load(os.path.join(GOLDEN, "sr_d.npz"))
    assert d["clear_in_file"].tobytes() == np.load(os.path.join(GOLDEN, "tr_d.npz"))["clear"].tobytes()


def test_literal_interval_list_equals_the_closed_forms():
    rng = np.random.default_rng(31)
    for trial in range(4000):
        grid = int(rng.choice([1, 5, 25]))
        n = int(rng.integers(1, 12))
        lo = rng.integers(0, 40, n) * grid
        if rng.random() < 0.15:
            lo[rng.integers(0, n)] = 0
        size = rng.integers(0, 6, n) * grid * (rng.random(n) < 0.8)
        pairs = [(int(a), int(a + s)) for a, s in zip(lo, size)]
        L = SR.IntervalList()
        for a, b in pairs:
            L.add(a, b - a)
        L.merge(0)
        merged = [tuple(e) for e in L.list]
        assert merged == SR.closed_merge_counts(pairs), pairs
        # the inversion of a merged list over a clear range around it, and the largest piece
        regions = [(a, b) for a, b, _ in merged]
        cb = int(rng.integers(0, regions[0][0] + 1))
        ce = regions[-1][1] + int(rng.integers(0, 4)) * grid
        assert SR.trim_bad_interval(regions, cb, ce) == SR.closed_largest_good(regions, cb, ce), (regions, cb, ce)


def test_round_is_half_away_from_zero():
    assert [SR.c_round(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 2.4999999999999996)] == [0, 0, 1, 2, 3, 2]
    # (1 / 2m) * m falls on one half or just below it; both occur
    below = sum((1 / (2 * m)) * m < 0.5 for m in range(252, 402))
    assert 0 < below < 150


def test_bad_input():
    lengths = [2000, 2000, 2000]
    one = lambda *r: np.array([r], dtype=REC)  # noqa: E731
    for rec, clear in ((one(4, 1, 0, 0), None), (one(1, 0, 0, 0), None), (one(1, 2, 1200 | (800 << 21), 0), None),
                       (one(1, 2, 0, 1200 | (800 << 21)), None), (one(1, 2, 0, 0), ([0, 900, 0], [2000, 800, 2000])),
                       (one(1, 2, 0, 0), ([0, 0, 0], [2000, 2001, 2000])),
                       (np.array([(2, 1, 0, 0), (1, 2, 0, 0)], dtype=REC), None),
                       (np.array([(1, 3, 0, 0), (1, 2, 0, 0)], dtype=REC), None)):
        with pytest.raises(SR.BadInput):
            SR.split_reads(lengths, rec, 3, clear, SR.Params())
    with pytest.raises(SR.BadInput):
        SR.split_reads([1 << 21], np.zeros(0, dtype=REC), 3, None, SR.Params())
    for raw in (b"", b"\x01\x00", struct.pack("<I", 1) + b"\0" * 12, struct.pack("<I", 2) + b"\0" * 16):
        with pytest.raises(ValueError):
            SR.parse_clear(raw, 1)


def split_result(R, TP, records):
    from canu_amd.split_reads import REGION_DTYPE, SplitResult
    bad = np.flatnonzero(R["fate"] >= SR.F_MANY)
    errs = np.stack([R["fate"][bad].astype(np.int64), records["a"][bad].astype(np.int64),
                     records["b"][bad].astype(np.int64)], axis=1)
    return SplitResult(params=TP, lengths=R["lengths"], clear_in=R["clear_in"], bgn=R["bgn"], end=R["end"],
                       status=R["status"], n_adjusted=R["n_adjusted"], n_bad_regions=R["n_bad_regions"],
                       fate=R["fate"], regions=np.array(R["regions"], dtype=REGION_DTYPE),
                       region_off=R["region_off"], error_pairs=errs, counters=R["counters"],
                       id_min=R["id_min"], id_max=R["id_max"], stats={})


def test_python_texts_equal_the_restatement():
    """canu_amd.split_reads.SplitResult writes the same bytes (no GPU needed for the writers)."""
    from canu_amd.split_reads import SrParameters, _clear_arrays, parse_splitReads_args
    for name in FIXTURES:
        fx, args, TP, P, rng, e0 = load(name)
        R = restate(fx, P, rng)
        res = split_result(R, TP, fx["records"])
        assert res.clear_bytes(entry0=e0) == fx["clear"].tobytes()
        assert res.log_text().encode() == fx["log"].tobytes()
        assert res.stats_text().encode() == fx["stats"].tobytes()
        assert res.stderr_text().encode() == fx["stderr"].tobytes()
        assert res.clear_bytes(existing=fx["clear"].tobytes(), entry0=e0) == fx["clear"].tobytes()
        with pytest.raises(ValueError):
            res.clear_bytes(existing=fx["clear"].tobytes()[:-4])
        # the three forms run() takes the input clear ranges in
        n = res.num_reads
        b, e = _clear_arrays(fx["clear"].tobytes(), n)
        assert np.array_equal(b, res.clear_ranges()[0]) and np.array_equal(e, res.clear_ranges()[1])
        b2, e2 = _clear_arrays(res, n)
        assert np.array_equal(b, b2) and np.array_equal(e, e2)
        assert _clear_arrays(None, n) is None
        with pytest.raises(ValueError):
            _clear_arrays((b[:-1], e[:-1]), n)
    ok = ["-G", "g", "-O", "o", "-Co", "c", "-o", "p"]
    for bad in (["-q"], ["-ol", "40"], ["-oc", "1"], ["-Cm", "x"], ["-t"], ["-e", "-1"]):
        with pytest.raises(ValueError):
            parse_splitReads_args(ok + bad)
    for k in (0, 2, 4, 6):                              # no -G, no -O, no -Co, no -o
        with pytest.raises(ValueError):
            parse_splitReads_args(ok[:k] + ok[k + 2:])
    P, job = parse_splitReads_args(ok + ["-Ci", "in", "-t", "3-9", "-minlength", "500", "-e", "0.04"])
    assert (job["clear_in"], job["id_min"], job["id_max"], P.min_read_length, P.erate) == ("in", 3, 9, 500, 0.04)
    assert parse_splitReads_args(ok)[1]["clear_in"] is None
    assert isinstance(SrParameters().to_c().erate, float)


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/sr_host_check.cpp, a program of its own with -fsanitize=address,undefined, on every
    fixture's bytes, on the libraries parser and on damaged clear range files."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "sr_host_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "sr_host_check.cpp")], check=True)
    for name in FIXTURES:
        fx, args, TP, P, rng, e0 = load(name)
        R = restate(fx, P, rng)
        d = tmp_path / name
        d.mkdir()
        (d / "args.txt").write_text("\n".join(args) + "\n")
        for k in ("lengths", "bgn", "end"):
            R[k].astype("<u4").tofile(d / f"{k}.bin")
        R["clear_in"][0].astype("<u4").tofile(d / "clear_bgn.bin")
        R["clear_in"][1].astype("<u4").tofile(d / "clear_end.bin")
        R["status"].astype(np.uint8).tofile(d / "status.bin")
        R["fate"].astype(np.uint8).tofile(d / "fate.bin")
        np.ascontiguousarray(fx["records"], dtype=REC).tofile(d / "records.bin")
        np.array([v for k in SR.COUNTERS for v in R["counters"][k]], dtype="<u8").tofile(d / "counters.bin")
        np.array(e0, dtype="<u4").tofile(d / "entry0.bin")
        (d / "want.clear").write_bytes(fx["clear"].tobytes())
        (d / "want.stats").write_bytes(fx["stats"].tobytes())
        (d / "want.errors").write_bytes(fx["stderr"].tobytes().split(b"\n", 1)[1])
        if "gkp_file_libraries" in fx.files:
            raw = fx["gkp_file_libraries"].tobytes()
            (d / "libraries").write_bytes(raw)
            flags = []
            for l in range(3):                          # library 0 is the store's empty record
                sw = struct.unpack_from("<3I", raw, 168 * l + 152)
                flags.append((1 if any(sw) else 0) | (2 if sw[2] else 0))
            assert flags[1:] == [3, 3]                  # what tools/make_sr_golden.py set
            np.array(flags, dtype=np.uint8).tofile(d / "lib_flags.bin")
        cp = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert cp.returncode == 0, (name, cp.stdout, cp.stderr)


def test_restatement_equals_the_reference_on_fresh_jobs(tmp_path):
    """Where the reference's objects are built (oracle/_ref): the reference splitReads, compiled out
    of tree, on random jobs it has not seen."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle
    import make_sr_golden as MS
    if not (oracle.reference_available() and oracle.store_available() and os.path.isdir(MS.REF)):
        pytest.skip("the reference is not built here")
    import test_gpu_sr as G
    binary = MS.build_reference(str(tmp_path))
    switches = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1)]          # lib_flags 0, 1, 3, 3
    for seed, ml in ((101, 0), (102, 64), (103, 1000)):
        lens, rec, libs, clear = G.random_job(seed)
        lib_of = [{0: 1, 1: 2, 3: 3 + (k & 1)}[int(f)] for k, f in enumerate(libs)]
        args = ["-e", "0.015", "-minlength", str(ml)]
        fx = MS.run_reference(binary, [int(v) for v in lens], [tuple(int(v) for v in r) for r in rec], lib_of,
                              switches, clear, args)
        assert np.array_equal(fx["lib_flags"], libs)
        P = SR.Params(0.015, ml)
        R = SR.split_reads(fx["lengths"], fx["records"], fx["lib_flags"], tuple(fx["clear_in"]), P)
        assert SR.clear_bytes(R) == fx["clear"].tobytes()
        assert fx["log"].tobytes() == b""
        assert SR.stats_text(R, P).encode() == fx["stats"].tobytes()
        assert SR.stderr_text(R, P, fx["records"]).encode() == fx["stderr"].tobytes()
        assert R["regions"] or seed != 101


def test_abi_header_and_binding_agree():
    """Every function include/canu_sr.h declares is bound, the built library exports it, and the
    structures have the sizes the header gives them."""
    import ctypes
    import re
    from canu_amd import split_reads as S
    src = open(os.path.join(ROOT, "include", "canu_sr.h")).read()
    assert sorted(set(re.findall(r"\b(sr_[a-z_]+)\s*\(", src))) == sorted(S.EXPORTS)
    assert int(re.search(r"#define SR_ABI_VERSION (\d+)", src).group(1)) == S.ABI_VERSION
    lib = ctypes.CDLL(S.LIB_PATH)
    assert not [e for e in S.EXPORTS if not hasattr(lib, e)]
    assert lib.sr_abi_version() == S.ABI_VERSION
    lib.sr_wave_capacity.restype = ctypes.c_uint32
    cap = lib.sr_wave_capacity()
    assert cap >= 128 and cap & (cap - 1) == 0
    assert ctypes.sizeof(S._Stats) == 20 * 16 + 8 + 5 * 8 + 3 * 8
    assert ctypes.sizeof(S._Params) == 16 and ctypes.sizeof(S._Result) == 9 * 8
    assert S.REGION_DTYPE.itemsize == 12
    for name, value in (("SR_LIB_ELIGIBLE", S.LIB_ELIGIBLE), ("SR_LIB_SUBREADS", S.LIB_SUBREADS),
                        ("SR_RECORDS_ON_DEVICE", S.RECORDS_ON_DEVICE), ("SR_CLEAR_ON_DEVICE", S.CLEAR_ON_DEVICE)):
        assert int(re.search(rf"#define {name}\s+(\d+)", src).group(1)) == value
    for name, value in (("SR_DELETED_OUT", S.DELETED_OUT), ("SR_TRIMMED", S.TRIMMED),
                        ("SR_FATE_SAME_ORIENT", S.FATE_SAME_ORIENT), ("SR_ERR_BAD_INPUT", -4)):
        assert int(re.search(rf"{name} = (-?\d+)", src).group(1)) == value
    # the header's own sizes, by the host compiler
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx):
        prog = ('#include "canu_sr.h"\n#include <cstdio>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(sr_stats), '
                'sizeof(sr_params), sizeof(sr_result), sizeof(sr_region));}\n')
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "s.cpp"), "w").write(prog)
            subprocess.run([cxx, "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"),
                            os.path.join(d, "s.cpp")], check=True)
            out = subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split()
        assert [int(v) for v in out] == [ctypes.sizeof(S._Stats), ctypes.sizeof(S._Params),
                                         ctypes.sizeof(S._Result), 12]
