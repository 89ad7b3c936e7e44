"""The host side of the aligner that overlapPair, falconsense and alignGFA share
(canu_amd/csrc/edlib_host.h), with no GPU: the sizes of a wave's path scratch and
obtainAlignment's leaf rule against the restatement the other tests pin to the reference."""
import os
import shutil
import subprocess

import pytest

import fs_restate as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF_BYTES = FS.LEAF_BYTES                      # FS_LEAF_BYTES, GFA_LEAF_BYTES
QUERIES = (1, 63, 64, 65, 4096, 4097)           # a block, a stripe, and one row more
TARGETS = (16384, 16385)                        # the last boundary row in LDS, the first in memory
LDS_COLUMNS = 16384
STRIPE_ROWS = 4096


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/edlib_host_check.cpp under AddressSanitizer and UBSan, a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("edlib_host") / "edlib_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "edlib_host_check.cpp")], check=True, timeout=300)
    return exe


def _lines(exe, *args):
    cp = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    return [[int(v) for v in ln.split()] for ln in cp.stdout.splitlines()]


def test_path_scratch_sizes(host_check):
    """Two rows of end blocks with one to spare, an operation buffer for q + t operations in
    16-byte steps, and a boundary row in memory only past LDS_COLUMNS."""
    cases = [(q, t) for q in QUERIES for t in TARGETS]
    got = _lines(host_check, "sizes", LEAF_BYTES, *[v for c in cases for v in c])
    assert len(got) == len(cases)
    for (q, t), (entries, blocks, ops, grow, grow_t, lds, stripe) in zip(cases, got):
        assert (lds, stripe) == (LDS_COLUMNS, STRIPE_ROWS)
        assert entries == LEAF_BYTES // 20 + 1
        assert blocks == -(-q // 64) + 1
        assert ops == (q + t + 64 + 15) // 16 * 16 and ops >= q + t + 64
        assert grow == grow_t == (0 if t <= LDS_COLUMNS else -(-t // 16))
        assert grow == 0 or 16 * grow >= t                   # 2 bits a column, 16 columns a word
    by = dict(zip(cases, got))
    assert [by[q, 16384][1] for q in QUERIES] == [2, 2, 2, 3, 65, 66]
    assert by[1, 16384][3] == 0 and by[1, 16385][3] == 1025


def test_leaf_rule_on_both_sides_of_its_limit(host_check):
    """is_leaf against fs_restate.is_leaf at the last target that is a leaf and the first that
    is split, for every query; and the largest leaf fits the leaf scratch."""
    cases = []
    for q in QUERIES:
        nb = -(-q // 64)
        last = (LEAF_BYTES - 1) // (20 * nb + 8)             # 20 nb t + 8 t < LEAF_BYTES
        cases += [(q, last), (q, last + 1), (q, 1)]
    got = _lines(host_check, "leaf", LEAF_BYTES, *[v for c in cases for v in c])
    assert len(got) == len(cases)
    for (q, t), (leaf, entries) in zip(cases, got):
        assert bool(leaf) == FS.is_leaf(q, t), (q, t)
        if leaf:
            assert -(-q // 64) * t <= entries                # a block column each
    assert [g[0] for g in got] == [1, 0, 1] * len(QUERIES)
