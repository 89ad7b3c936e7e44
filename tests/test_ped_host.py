"""The host side of the aligner that overlapInCore, findErrors and correctOverlaps share
(canu_amd/csrc/ped_host.h), with no GPU: Edit_Match_Limit against the two restatements the
other tests pin to the reference, and the sizes of a wave's row log."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fe_restate as FR
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AS_MAX_READLEN = (1 << 21) - 1
ERATES = (0.045, 0.06, 0.144, 0.30)
UPTO = (0, 1, 2, 50, 1999, 2000, 2001)          # 2000: the switch to the linear tail
PER_ERROR = 128                                 # FE_LOG_PER_ERROR, CO_LOG_PER_ERROR


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/ped_host_check.cpp under AddressSanitizer and UBSan, a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("ped_host") / "ped_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "ped_host_check.cpp")], check=True, timeout=300)
    return exe


def _lines(exe, *args):
    cp = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    return [[int(v) for v in ln.split()] for ln in cp.stdout.splitlines()]


def test_match_limit_equals_the_restatements(host_check):
    """init_match_limit as findErrors and correctOverlaps call it (max_errors truncated, the table
    up to `upto`) and as overlapInCore does (max_errors rounded up, upto = max_errors)."""
    cases = [(e, 1 + int(e * AS_MAX_READLEN), u) for e in ERATES for u in UPTO]
    ovl_erate = float(np.float32(0.06))                      # overlapInCore parses a float
    ovl_me = 1 + math.ceil(ovl_erate * AS_MAX_READLEN)
    cases.append((ovl_erate, ovl_me, ovl_me))
    got = _lines(host_check, "limit", *[repr(v) for c in cases for v in c])
    assert len(got) == len(cases)
    restated = {e: (FR.match_limit(e, max(UPTO) + 1), oracle.match_limit(e, max(UPTO) + 1)[1])
                for e in ERATES}
    for (erate, me, upto), ml in zip(cases[:-1], got):
        assert upto < me and len(ml) == upto + 1
        for ref in restated[erate]:
            assert ml == ref[:upto + 1].tolist(), (erate, upto)
    me, lim = oracle.match_limit(ovl_erate, ovl_me + 1)
    assert me == ovl_me and got[-1] == lim.tolist()
    assert got[-1][ovl_me - 1] > 0 and got[-1][ovl_me] == 0  # filled below max_errors only


def test_row_log_sizes(host_check):
    """(limit + 1)^2 + 64 at the worst, per_error values per error at first where that is less,
    and no regrowing of a log that was the worst case already."""
    cross = next(l for l in range(1, 1 << 20) if (l + 1) ** 2 + 64 > PER_ERROR * l + 64)
    limits = [0, 1, cross - 1, cross]
    got = _lines(host_check, "sizes", PER_ERROR, *limits)
    for limit, (rows, worst, first, grown, grown_worst, log_max) in zip(limits, got):
        assert rows == sum(2 * e + 1 for e in range(limit + 1)) == (limit + 1) ** 2
        assert worst == rows + 64
        assert first == min(PER_ERROR * limit + 64, worst)
        assert grown == (0 if first >= rows else worst)
        assert grown_worst == 0
        assert log_max == 0x7fff0000
    by = dict(zip(limits, got))
    assert by[0][2] == 64 and by[1][2] == 4 + 64             # at 1 the worst case is the smaller
    assert by[cross - 1][2] == by[cross - 1][1] and by[cross][2] == PER_ERROR * cross + 64 < by[cross][1]
