"""trimReads without a GPU: the restatement (tests/tr_restate.py) against the reference's own
files (tests/golden/tr_*.npz, tools/make_tr_golden.py), the literal intervalList against the
closed forms the kernel computes, the branches the fixtures reach, and the host code of the
drop-in executable under the sanitizers (tests/tr_host_check.cpp)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tr_restate as TR  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("a", "b0", "b1", "b2", "b3", "c", "d")


def load(name):
    fx = np.load(os.path.join(GOLDEN, f"tr_{name}.npz"))
    args = fx["args"].tobytes().decode().split()
    kv = dict(zip(args[0::2], args[1::2]))
    P = TR.Params(float(kv["-e"]), int(kv["-minlength"]), int(kv["-ol"]), int(kv["-oc"]))
    rng = tuple(int(v) for v in kv["-t"].split("-")) if "-t" in kv else None
    return fx, args, P, rng


@pytest.mark.parametrize("closed", [False, True], ids=["literal", "closed"])
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(name, closed):
    fx, _, P, rng = load(name)
    R = TR.trim_reads(fx["lengths"], fx["records"], fx["rules"], P, rng, closed=closed)
    assert TR.clear_bytes(R) == fx["clear"].tobytes()
    assert TR.log_text(R).encode() == fx["log"].tobytes()
    assert TR.stats_text(R, P).encode() == fx["stats"].tobytes()
    assert TR.stderr_text(R).encode() == fx["stderr"].tobytes()


def test_fixtures_hold_no_plot_text_and_are_small():
    for name in FIXTURES:
        path = os.path.join(GOLDEN, f"tr_{name}.npz")
        assert os.path.getsize(path) < 64 * 1024, name
        fx = np.load(path)
        for k in fx.files:
            if fx[k].dtype == np.uint8:
                raw = fx[k].tobytes()
                assert b"set terminal" not in raw and b"plot " not in raw and b"binwidth" not in raw, (name, k)
        assert not any(str(f).endswith((".gp", ".dat")) for k in fx.files if k.endswith("_names") for f in fx[k])


def test_fixtures_reach_the_required_branches():
    br = {}
    for name in FIXTURES:
        fx, _, P, rng = load(name)
        TR.trim_reads(fx["lengths"], fx["records"], fx["rules"], P, rng, branches=br)
    missing = [b for b in TR.REQUIRED_BRANCHES if not br.get(b)]
    assert not missing, missing
    # what is argued to be unreachable is not reached
    assert "be_update_end_fails" not in br and "be_clamp" not in br


def _random_set(rng):
    n = int(rng.integers(1, 14))
    span = int(rng.choice([20, 60, 300, 3000]))
    ivs = []
    for _ in range(n):
        lo = int(rng.integers(0, span + 1))
        if rng.random() < 0.15:
            lo = 0
        hi = lo + int(rng.integers(1, span + 1))
        ivs.append((lo, hi, int(rng.choice([0, 0, 0, 0, 500]))))
        if rng.random() < 0.2:
            ivs.append(ivs[-1])                         # duplicates
        if rng.random() < 0.2:
            ivs.append((hi, hi + int(rng.integers(1, span + 1)), 0))   # touching ends
    return ivs


def test_literal_interval_list_equals_the_closed_forms():
    """A few thousand random sets: hi below minOverlap, duplicates, touching ends, minOverlap
    0 / 1 / 40, minCoverage 0 .. 4."""
    rng = np.random.default_rng(123)
    n_literal = n_wrap = n_differs = 0
    for it in range(4000):
        ivs = _random_set(rng)
        ol, oc = int(rng.choice([0, 1, 40])), int(rng.integers(0, 5))
        used = [(a, b) for a, b, e in ivs if e <= 150]
        assert TR.largest_covered(ivs, 150, ol, oc) == TR.largest_covered_closed(ivs, 150, ol, oc), (ivs, ol, oc)
        if not used:
            continue
        L = TR.IntervalList()
        for a, b in used:
            L.add(a, b - a)
        if oc > 0:
            lit = [(lo, hi) for lo, hi, _ in TR.depth_regions(L, oc).list]
            if TR.depth_needs_literal(used, oc):
                n_literal += 1
                n_differs += lit != TR.closed_depth_runs(used, oc)
            else:
                assert lit == TR.closed_depth_runs(used, oc), (used, oc)
        L.merge(ol)
        assert [(lo, hi) for lo, hi, _ in L.list] == TR.closed_merge(used, ol), (used, ol)
        n_wrap += any(b < ol for _, b in used)
    # the sets reach the uint32 wrap, the literal walk, and sets where the reference's depth list
    # is not the true depth
    assert n_wrap > 100 and n_literal > 100 and n_differs > 0, (n_wrap, n_literal, n_differs)


def test_depth_list_is_not_the_true_depth():
    """computeDepth folds [300, 300) back into [100, 300) and the second close lowers that piece
    to 1: with -oc 2 nothing is left, though 100 .. 300 is covered twice (fixture b2 holds the
    reference's answer)."""
    ivs = [(0, 300, 0), (100, 300, 0), (300, 400, 0)]
    assert TR.closed_depth_runs([(a, b) for a, b, _ in ivs], 2) == [(100, 300)]
    assert TR.largest_covered(ivs, 150, 40, 2)[0] is False
    assert TR.largest_covered_closed(ivs, 150, 40, 2)[0] is False
    assert TR.largest_covered(ivs, 150, 40, 1)[:3] == (True, 0, 300)


def test_b_iid_tie_break_does_not_reach_the_output():
    rng = np.random.default_rng(8)
    for name in ("c", "d"):
        fx, _, P, r = load(name)
        rec = fx["records"].copy()
        one = TR.trim_reads(fx["lengths"], rec, fx["rules"], P, r)
        two = TR.trim_reads(fx["lengths"], rec, fx["rules"], P, r, ignore_b_iid=True)
        rec["b"] = rng.integers(1, 4, rec.shape[0])     # many equal b_iid: the tie-break fires
        three = TR.trim_reads(fx["lengths"], rec, fx["rules"], P, r)
        for other in (two, three):
            assert TR.log_text(one) == TR.log_text(other) and TR.clear_bytes(one) == TR.clear_bytes(other)


def test_bad_input():
    rec = np.array([TR.make_record(2, 1, 0, 500, 1000), TR.make_record(1, 2, 0, 500, 1000)],
                   dtype=[("a", "<u4"), ("b", "<u4"), ("w0", "<u8"), ("w1", "<u8")])
    with pytest.raises(TR.BadInput):
        TR.trim_reads([1000, 1000], rec, 1, TR.Params())
    with pytest.raises(TR.BadInput):
        TR.trim_reads([1000], rec[:1], 1, TR.Params())
    with pytest.raises(TR.BadInput):
        TR.trim_reads([1000, 1000], rec[1:], 0, TR.Params())
    for raw in (b"", b"\x01\0\0", b"\x01\0\0\0" + b"\0" * 15, b"\x02\0\0\0" + b"\0" * 16):
        with pytest.raises(ValueError):
            TR.parse_clear(raw, 1)


def test_python_texts_equal_the_restatement():
    """canu_amd.trim_reads.TrimResult writes the same bytes (no GPU needed for the writers)."""
    from canu_amd.trim_reads import TrimResult, TrParameters, parse_trimReads_args
    for name in FIXTURES:
        fx, args, P, rng = load(name)
        R = TR.trim_reads(fx["lengths"], fx["records"], fx["rules"], P, rng)
        TP, job = parse_trimReads_args(args + ["-G", "g", "-O", "o", "-Co", "c", "-o", "p"])
        assert (TP.erate, TP.min_read_length, TP.min_evidence_overlap, TP.min_evidence_coverage) == \
            (P.erate, P.min_read_length, P.min_evidence_overlap, P.min_evidence_coverage)
        res = TrimResult(params=TP, lengths=R["lengths"], bgn=R["bgn"], end=R["end"], status=R["status"],
                         flags=(R["no_hq"] | (R["reset"] << 1)).astype(np.uint8), n_skipped=R["n_skipped"],
                         n_used=R["n_used"], counters=R["counters"], id_min=R["id_min"], id_max=R["id_max"],
                         stats={})
        assert res.clear_bytes() == fx["clear"].tobytes()
        assert res.log_text().encode() == fx["log"].tobytes()
        assert res.stats_text().encode() == fx["stats"].tobytes()
        assert res.stderr_text().encode() == fx["stderr"].tobytes()
        assert res.clear_bytes(existing=fx["clear"].tobytes()) == fx["clear"].tobytes()
    for bad in (["-Ci", "x"], ["-Cm", "x"], ["-l", "40"], ["-q"]):
        with pytest.raises(ValueError):
            parse_trimReads_args(["-G", "g", "-O", "o", "-Co", "c", "-o", "p"] + bad)
    with pytest.raises(ValueError):
        parse_trimReads_args(["-G", "g", "-O", "o", "-o", "p"])
    assert isinstance(TrParameters().to_c().erate, float)


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/tr_host_check.cpp, a program of its own with -fsanitize=address,undefined, on every
    fixture's bytes and on damaged clear range files."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "tr_host_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "tr_host_check.cpp")], check=True)
    for name in FIXTURES:
        fx, args, P, rng = load(name)
        R = TR.trim_reads(fx["lengths"], fx["records"], fx["rules"], P, rng)
        d = tmp_path / name
        d.mkdir()
        (d / "args.txt").write_text("\n".join(args) + "\n")
        for k in ("lengths", "bgn", "end", "n_skipped", "n_used"):
            R[k].astype("<u4").tofile(d / f"{k}.bin")
        R["status"].astype(np.uint8).tofile(d / "status.bin")
        (R["no_hq"] | (R["reset"] << 1)).astype(np.uint8).tofile(d / "flags.bin")
        np.array([v for k in TR.COUNTERS for v in R["counters"][k]], dtype="<u8").tofile(d / "counters.bin")
        np.array([R["id_min"], R["id_max"]], dtype="<u4").tofile(d / "range.bin")
        for ext in ("clear", "log", "stats"):
            (d / f"want.{ext}").write_bytes(fx[ext].tobytes())
        if "gkp_file_libraries" in fx.files:
            (d / "libraries").write_bytes(fx["gkp_file_libraries"].tobytes())
            # library 0 is the store's empty record, a default gkLibrary: largestCovered
            np.array([1, 1, 2], dtype="<u4").tofile(d / "final_trim.bin")
        cp = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert cp.returncode == 0, (name, cp.stdout, cp.stderr)


def test_restatement_equals_the_reference_on_fresh_jobs(tmp_path):
    """Where the reference's objects are built (oracle/_ref): the reference trimReads, compiled out
    of tree, on random jobs it has not seen."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle
    import make_tr_golden as MT
    if not (oracle.reference_available() and oracle.store_available() and os.path.isdir(MT.REF)):
        pytest.skip("the reference is not built here")
    binary = MT.build_reference(str(tmp_path))
    for seed, rule, oc in ((1, 1, 2), (2, 2, 1), (3, 1, 3)):
        cases = MT.random_cases(9000 + seed, 40, grid=int(10 * seed))
        lens, recs = MT.hand_records(cases, len(cases) + 2)
        lens += [1000] * 5
        args = MT.CANU_ARGS + ["-oc", str(oc)]
        fx = MT.run_reference(binary, lens, recs, [1] * len(lens), [rule], args)
        P = TR.Params(0.015, 64, 40, oc)
        R = TR.trim_reads(fx["lengths"], fx["records"], fx["rules"], P)
        assert TR.clear_bytes(R) == fx["clear"].tobytes()
        assert TR.log_text(R).encode() == fx["log"].tobytes()
        assert TR.stats_text(R, P).encode() == fx["stats"].tobytes()
        assert TR.stderr_text(R).encode() == fx["stderr"].tobytes()


def test_abi_header_and_binding_agree():
    """Every function include/canu_tr.h declares is bound, and the built library exports it."""
    import ctypes
    import re
    from canu_amd import trim_reads as T
    src = open(os.path.join(ROOT, "include", "canu_tr.h")).read()
    assert sorted(set(re.findall(r"\b(tr_[a-z_]+)\s*\(", src))) == sorted(T.EXPORTS)
    assert int(re.search(r"#define TR_ABI_VERSION (\d+)", src).group(1)) == T.ABI_VERSION
    lib = ctypes.CDLL(T.LIB_PATH)
    assert not [e for e in T.EXPORTS if not hasattr(lib, e)]
    assert lib.tr_abi_version() == T.ABI_VERSION
    assert ctypes.sizeof(T._Stats) == 9 * 16 + 8 + 5 * 8 + 3 * 8
