"""falconsense without a GPU: the Python restatement (tests/fs_restate.py) against the reference's
output in the fixtures, the branches the fixtures reach, the integer form of the scan, and the
host code (corStore reader, FASTA writer) as a sanitizer build of its own."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fs_restate as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def runs():
    """Every fixture through the restatement, once: name -> (stdout, stderr, branch log)."""
    out = {}
    for name in FS.FIXTURES:
        log = FS.new_log()
        o, e = FS.run_golden(FS.golden(name), log)
        out[name] = (o, e, log)
    return out


@pytest.mark.parametrize("name", FS.FIXTURES)
def test_restatement_equals_reference(runs, name):
    g = FS.golden(name)
    o, e, _ = runs[name]
    assert e == g["stderr"]
    assert o == g["stdout"]


@pytest.mark.parametrize("name", FS.FIXTURES)
def test_corstore_decodes(name):
    g = FS.golden(name)
    lay, kids = FS.decode_corstore(g["tig"], g["dat"])
    assert np.array_equal(lay, g["layouts"]) and np.array_equal(kids, g["children"])


def test_fixtures_reach_the_branches(runs):
    tot = FS.new_log()
    for _, _, log in runs.values():
        for k, v in log.items():
            tot[k] = max(tot[k], v) if k == "max_depth" else tot[k] + v
    assert tot["leaf"] > 0
    assert tot["max_depth"] >= 2
    assert tot["rejected"] > 0
    assert tot["skipped"] > 0
    assert tot["truncated"] > 0
    assert tot["tie_first_appearance"] > 0
    assert tot["n_link"] > 0
    assert tot["dropped_first"] > 0
    assert tot["empty_output"] > 0
    for name, (_, _, log) in runs.items():
        assert (log["aligned"], log["skipped"], log["rejected"]) == FS.EXPECTED_COUNTS[name], name
    # the exclusive end and the -r list: fixture e names reads 1, 2, 4, 7, 9 and runs -b 2 -e 7
    assert runs["e"][1].count(b"Processing read") == 2
    # several pieces from one template
    assert b">read2_1\n" in runs["f"][0]


def _cost(ops: bytes) -> int:
    return sum(1 for o in ops if o != FS.MATCH)


def test_boundary_split_rules():
    """Real reads do not reach the two boundary rules of the split (the whole query on one side of
    the target's middle): the path function is given such pairs directly.  Only this restatement
    covers them: an infix alignment never starts or ends with a deleted target base, so no
    layout hands the device such a pair at the top, and below it the halves follow the data."""
    rng = np.random.default_rng(5)
    q = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, 1700)].tobytes()
    junk = np.frombuffer(b"GT", dtype=np.uint8)[rng.integers(0, 2, 1700)].tobytes()
    for t, key in ((junk + q, "split_top"), (q + junk, "split_bottom")):
        log = FS.new_log()
        assert not FS.is_leaf(len(q), len(t))
        ops = FS.path(q, t, 1700, log)
        assert log[key] == 1 and log["empty_side"] >= 1
        assert _cost(ops) == 1700
        assert sum(o != FS.DELETE for o in ops) == len(q) and sum(o != FS.INSERT for o in ops) == len(t)


def test_path_is_an_alignment():
    rng = np.random.default_rng(6)
    t = _ACGT[rng.integers(0, 4, 2600)].tobytes()
    q = bytearray(t[300:2300])
    for p in sorted(rng.integers(0, len(q), 200).tolist(), reverse=True):
        if p % 3 == 0:
            del q[p]
        elif p % 3 == 1:
            q.insert(p, 65)
        else:
            q[p] = 67 if q[p] != 67 else 71
    q = bytes(q)
    d, s, e = FS.locate(q, t, 10 ** 6)
    log = FS.new_log()
    ops = FS.path(q, t[s:e + 1], d, log)
    assert log["split"] >= 1 and log["leaf"] >= 2
    i = j = cost = 0
    for o in ops:
        if o in (FS.MATCH, FS.MISMATCH):
            assert (q[i] == t[s + j]) == (o == FS.MATCH)
            i += 1
            j += 1
        elif o == FS.INSERT:
            i += 1
        else:
            j += 1
        cost += o != FS.MATCH
    assert (i, j, cost) == (len(q), e - s + 1, d)


def _random_tags(rng, tlen, n_ev):
    """Tag lists of random alignments against a template of tlen bases."""
    out = []
    for _ in range(n_ev):
        b = int(rng.integers(0, tlen // 2))
        e = int(rng.integers(b + 2, tlen + 1))
        ops = bytearray()
        for _ in range(e - b):
            while rng.random() < 0.15:
                ops.append(FS.INSERT)
            ops.append(FS.DELETE if rng.random() < 0.1 else FS.MATCH)
        q = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, len(ops))].tobytes()
        out.append(FS.align_tags(bytes(ops), q, b))
    return out


@pytest.mark.parametrize("seed", range(12))
def test_integer_scan_equals_double_scan(seed):
    rng = np.random.default_rng(1000 + seed)
    tlen = int(rng.integers(20, 120))
    tags = _random_tags(rng, tlen, int(rng.integers(1, 9)))
    for min_cov in (0, 2, 4):
        assert FS.consensus_int(tags, tlen, min_cov) == FS.consensus(tags, tlen, min_cov)


def test_atoi_identity_and_selection():
    o = FS.parse_args(["-G", "g", "-C", "c", "-b", "3", "-e", "9", "-ci", "0.85", "-cc", "4"])
    assert o["ci"] == 0.0 and (o["bgn"], o["end"]) == (3, 9)
    assert FS.selected(o, 6, None) == [3, 4, 5]            # the end is clamped and exclusive
    assert FS.selected(o, 20, [1, 4, 9, 12]) == [4]        # 9 is listed, kept, and never reached


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_code_under_sanitizers(tmp_path):
    """tests/fs_host_check.cpp, built with -fsanitize=address,undefined and run directly: the
    corStore reader on the fixtures' stores, their truncations and damaged counts, and the FASTA
    writer's 60-column rule."""
    exe = tmp_path / "fs_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "fs_host_check.cpp")], check=True)
    names = []
    for name in FS.FIXTURES:
        g = FS.golden(name)
        (tmp_path / f"{name}.tig").write_bytes(g["tig"])
        (tmp_path / f"{name}.dat").write_bytes(g["dat"])
        lay, kids = g["layouts"], g["children"]
        exp = struct.pack("<I", len(lay)) + b"".join(
            struct.pack("<IIII", *(int(v) for v in l)) for l in lay)
        exp += struct.pack("<I", len(kids)) + b"".join(
            struct.pack("<IIiiii", *(int(v) for v in k)) for k in kids)
        (tmp_path / f"{name}.expect").write_bytes(exp)
        names.append(name)
    cp = subprocess.run([str(exe), str(tmp_path), *names], capture_output=True, text=True)
    assert cp.returncode == 0, cp.stderr[-3000:]
    assert f"{len(names)} store(s) ok" in cp.stdout


def test_header_declares_the_python_exports():
    import re
    from canu_amd import falconsense as F
    src = open(os.path.join(ROOT, "include", "canu_fs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(fs_[a-z_]+)\s*\(", src))) == sorted(F.EXPORTS)
    assert int(re.search(r"#define FS_ABI_VERSION (\d+)", src).group(1)) == F.ABI_VERSION
    assert int(re.search(r"#define FS_LEAF_BYTES (\d+)", src).group(1)) == F.LEAF_BYTES == FS.LEAF_BYTES
    assert int(re.search(r"#define FS_MIN_EVIDENCE (\d+)", src).group(1)) == F.MIN_EVIDENCE == FS.MIN_EVIDENCE
