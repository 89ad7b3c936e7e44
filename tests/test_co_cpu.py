"""correctOverlaps' host side, with no GPU: the Python restatement against the reference's
fixtures, what the fixtures cover, the argument line, the .oea helpers and the file readers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import co_restate as CR
import fe_restate as FR
from canu_amd import correct_overlaps as CO
from canu_amd.overlap_in_core import RECORD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_restated: dict = {}


def restated(name):
    """A fixture through the restatement, once -> (evalues, counters, branches)."""
    if name not in _restated:
        g = CR.golden(name)
        br: dict = {}
        ev, c = CR.correct_overlaps(g["records"], FR.reads_dict(g["rs"]), g["red"], g["bgn"],
                                    g["end"], g["erate"], br)
        ev.setflags(write=False)
        _restated[name] = (ev, c, br)
    return _restated[name]


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_restatement_equals_reference(name):
    """Pins tests/co_restate.py to the reference correctOverlaps: the .oea bytes, the nine
    counters and the numbers of the "Corrected" line."""
    g = CR.golden(name)
    ev, c, _ = restated(name)
    assert CR.oea_bytes(g["bgn"], g["end"], ev) == g["oea"]
    assert c == g["counters"]


def test_fixtures_cover_the_cases():
    """What the fixtures are for, on the reference's own output and on the paths the pinned
    restatement takes through them."""
    branches: dict = {}
    raised = lowered = kept = 0
    names = []
    for n in CR.FIXTURES:
        g = CR.golden(n)
        ev, c, br = restated(n)
        for k, v in br.items():
            branches[k] = branches.get(k, 0) + v
        bgn, end, cnt = CO.parse_oea(g["oea"])
        assert (bgn, end) == (g["bgn"], g["end"]) and cnt.shape[0] == g["records"].shape[0]
        came = CO.evalues_of(g["records"])
        assert came.min() > 0 and np.unique(came).shape[0] >= came.shape[0] // 2   # twins share one
        raised += int((cnt > came).sum())
        lowered += int((cnt < came).sum())
        kept += int((cnt == came).sum())
        c = g["counters"]
        assert c["total"] == c["olaps_fwd"] + c["olaps_rev"] == cnt.shape[0]
        assert c["olaps_fwd"] > 0 and c["olaps_rev"] > 0, n
        if c["failed_either"] > c["failed_both"]:
            names.append(n)
        # a failed overlap keeps its evalue; distinct evalues make that visible
        assert int((cnt == came).sum()) >= c["failed_either"]
    missing = [k for k in CR.REQUIRED_BRANCHES if not branches.get(k)]
    assert not missing, missing
    assert names, "no fixture where an alignment fails one test and not the other"
    assert raised > 0 and lowered > 0 and kept > 0
    tot = {k: sum(CR.golden(n)["counters"][k] for n in CR.FIXTURES) for k in CR.COUNTERS + CR.CORRECTED}
    assert tot["rha_fail"] > 0 and tot["rha_pass"] > 0
    assert tot["insertions"] > 0 and tot["deletions"] > 0 and tot["substitutions"] > 0
    a, b, c, d = (CR.golden(n) for n in "abcd")
    assert a["erate"] == 0.045 and b["erate"] == 0.144
    t = (c["red"]["word"] >> 2) & 15
    key = (c["red"]["readID"].astype(np.uint64) << np.uint64(32)) | (c["red"]["word"] >> 6)
    _, n2 = np.unique(key[t != 0], return_counts=True)
    assert (n2 == 2).any() and (t >= FR.A_INSERT).any() and (t == FR.DELETE).any()
    assert b"N" in d["rs"].bases.tobytes()
    assert (d["records"]["b"] > d["end"]).any()                       # B outside the range
    ids = np.unique(d["red"]["readID"][(d["red"]["word"] >> 2) & 15 != 0])
    assert np.setdiff1d(np.unique(d["records"]["a"]), ids).size       # a read with no corrections
    HM = np.uint64((1 << 21) - 1)
    assert ((d["records"]["w0"] & HM) == (d["records"]["w1"] & HM)).any()   # a_hang == 0


def test_the_variant_aligner_is_not_findErrors():
    """correctOverlaps' Prefix_Edit_Dist fails with Error_Limit + 1 and no delta; findErrors'
    returns its best branch point.  On an overlap that leaves the read they differ."""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 4, 600).astype(np.uint8)
    b = np.concatenate([a[:300], rng.integers(0, 4, 300).astype(np.uint8)])
    ML = FR.match_limit(0.06, 64)
    e1 = CR.prefix_edit_dist(a, b, CR.error_bound(600, 0.06), ML)
    e2 = FR.prefix_edit_dist(a, b, FR.error_bound(600, 0.06), 0.06, ML)
    assert not e1[3] and not e2[3]
    assert e1[0] == CR.error_bound(600, 0.06) + 1 and e1[4] == [] and e2[0] <= 36


def test_parse_args():
    P, job = CO.parse_correctOverlaps_args(
        ["-G", "g", "-O", "o", "-R", "3", "9", "-e", "0.045", "-l", "500", "-c", "r.red", "-o",
         "1.oea", "-t", "8"])
    assert P.error_rate == 0.045
    assert job == {"gkp": "g", "ovl": "o", "red": "r.red", "out": "1.oea", "bgn": 3, "end": 9,
                   "threads": 8, "min_overlap": 500}
    P, job = CO.parse_correctOverlaps_args(["-G", "g", "-O", "o", "-c", "r", "-o", "x"])
    assert P.error_rate == 0.06 and (job["bgn"], job["end"]) == (0, 0xFFFFFFFF)
    assert CO.clamp_range(0, 0xFFFFFFFF, 70) == (1, 70) and CO.clamp_range(4, 9, 70) == (4, 9)
    for bad in (["-G", "g", "-O", "o", "-c", "r"], ["-G", "g", "-O", "o", "-o", "x"],
                ["-O", "o", "-c", "r", "-o", "x"], ["-G", "g", "-c", "r", "-o", "x"],
                ["-G", "g", "-O", "o", "-c", "r", "-o", "x", "-k", "9"],
                ["-G", "g", "-O", "o", "-c", "r", "-o"]):
        with pytest.raises(ValueError):
            CO.parse_correctOverlaps_args(bad)


def test_oea_round_trip(tmp_path):
    ev = np.array([0, 1, 4095, 450, 77], dtype=np.uint16)
    p = str(tmp_path / "1.oea")
    CO.write_oea(p, 3, 9, ev)
    raw = open(p, "rb").read()
    assert raw == struct.pack("<iiQ", 3, 9, 5) + ev.astype("<u2").tobytes()
    bgn, end, got = CO.read_oea(p)
    assert (bgn, end) == (3, 9) and np.array_equal(got, ev)
    CO.write_oea(p, 1, 2, np.zeros(0, dtype=np.uint16))
    assert CO.read_oea(p)[2].shape == (0,) and os.path.getsize(p) == 16
    g = CR.golden("a")
    assert CO.oea_bytes(*CO.parse_oea(g["oea"])) == g["oea"]
    for bad in (raw[:-1], raw + b"\0", raw[:15], b""):
        with pytest.raises(ValueError):
            CO.parse_oea(bad)


def test_report():
    g = CR.golden("b")
    text = CO.report(g["counters"])
    c = g["counters"]
    assert text.splitlines()[0] == (f"Corrected {c['corrected_bases']} bases with "
                                    f"{c['substitutions']} substitutions, {c['deletions']} "
                                    f"deletions and {c['insertions']} insertions.")
    assert f"Failed: {c['failed_either']} (either)\n" in text
    assert text.endswith(f"rhaFail {c['rha_fail']} rhaPass {c['rha_pass']}\n")
    assert len(text.splitlines()) == 9


def test_apply_evalues():
    g = CR.golden("c")
    rec = g["records"]
    ev = np.arange(rec.shape[0], dtype=np.uint16) % 4096
    out = CO.apply_evalues(rec, ev)
    assert np.array_equal(CO.evalues_of(out), ev)
    mask = ~(np.uint64(0xFFF) << np.uint64(42))
    assert np.array_equal(out["w0"] & mask, rec["w0"] & mask)
    for f in ("a", "b", "w1"):
        assert np.array_equal(out[f], rec[f])
    assert np.array_equal(CO.apply_evalues(rec, CO.evalues_of(rec)), rec)
    assert not np.shares_memory(out, rec)
    with pytest.raises(ValueError):
        CO.apply_evalues(rec, ev[:-1])
    with pytest.raises(ValueError):
        CO.apply_evalues(rec, ev.astype(np.int64) + 4096)
    assert CO.apply_evalues(np.zeros(0, dtype=RECORD_DTYPE), np.zeros(0, dtype=np.uint16)).shape == (0,)


def test_library_exports_and_header(built):
    lib = CO.load_library()
    assert not [e for e in CO.EXPORTS if not hasattr(lib, e)]
    assert lib.co_abi_version() == CO.ABI_VERSION
    p = CO._Params()
    lib.co_params_init(p)
    assert p.error_rate == 0.06
    hdr = open(os.path.join(ROOT, "include", "canu_co.h")).read()
    assert f"#define CO_WINDOW_DIAGS {CO.WINDOW_DIAGS}\n" in hdr
    assert f"#define CO_LOG_PER_ERROR {CO.LOG_PER_ERROR}\n" in hdr
    assert f"#define CO_LDS_BASES {CO.LDS_BASES}\n" in hdr
    assert f"#define CO_ABI_VERSION {CO.ABI_VERSION}\n" in hdr
    for code, name in CO.CO_STATUS.items():
        assert f"{name} = {code}" in hdr
    for e in CO.EXPORTS:
        assert e + "(" in hdr
    for n in CO.COUNTERS + CO.CORRECTED:
        assert n in hdr


# ----------------------------------------------------------------------- the file readers

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/co_host_check.cpp under AddressSanitizer and UBSan, a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("co_host") / "co_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "co_host_check.cpp")], check=True, timeout=300)
    return exe


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_file_readers_read_the_reference_files(host_check, tmp_path):
    for n in CR.FIXTURES:
        g = CR.golden(n)
        red, oea = str(tmp_path / f"{n}.red"), str(tmp_path / f"{n}.oea")
        open(red, "wb").write(g["red"].tobytes())
        open(oea, "wb").write(g["oea"])
        cp = _run(host_check, "red", red)
        assert cp.returncode == 0, cp.stderr
        assert cp.stdout == (f"red ok: {g['red'].shape[0]} records, "
                             f"{np.unique(g['red']['readID']).shape[0]} reads\n")
        ev = CO.parse_oea(g["oea"])[2]
        cp = _run(host_check, "copy", oea, oea + ".copy")
        assert cp.returncode == 0, cp.stderr
        assert cp.stdout == f"oea ok: {g['bgn']} {g['end']} {ev.shape[0]} {int(ev.sum())}\n"
        assert open(oea + ".copy", "rb").read() == g["oea"]
    empty = str(tmp_path / "empty.red")
    open(empty, "wb").close()
    assert _run(host_check, "red", empty).stdout == "red ok: 0 records, 0 reads\n"


def test_file_readers_refuse_damaged_files(host_check, tmp_path):
    g = CR.golden("a")
    red, oea = g["red"].tobytes(), g["oea"]
    swapped = g["red"].copy()
    k = int(np.nonzero(np.diff(swapped["readID"].astype(np.int64)) > 0)[0][0])
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    n = struct.unpack("<Q", oea[8:16])[0]
    cases = {
        "red mid record": ("red", red[:-3]),
        "red one byte": ("red", red[:1]),
        "red unsorted": ("red", swapped.tobytes()),
        "oea no header": ("oea", oea[:15]),
        "oea empty": ("oea", b""),
        "oea truncated": ("oea", oea[:-2]),
        "oea mid evalue": ("oea", oea[:-1]),
        "oea trailing": ("oea", oea + b"\0\0"),
        "oea count too large": ("oea", oea[:8] + struct.pack("<Q", n + 1) + oea[16:]),
        "oea count huge": ("oea", oea[:8] + struct.pack("<Q", (1 << 63) + 8) + oea[16:]),
        "oea count wraps": ("oea", oea[:8] + struct.pack("<Q", (1 << 64) - 8) + oea[16:]),
    }
    for name, (kind, data) in cases.items():
        p = str(tmp_path / (name.replace(" ", "_") + "." + kind))
        open(p, "wb").write(data)
        cp = _run(host_check, kind, p)
        assert cp.returncode == 2 and cp.stderr.startswith("error: "), (name, cp.returncode,
                                                                        cp.stderr[-400:])
    cp = _run(host_check, "red", str(tmp_path / "missing.red"))
    assert cp.returncode == 2 and cp.stderr.startswith("error: ")
