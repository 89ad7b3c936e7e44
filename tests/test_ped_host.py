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


N_CU = 256
WAVES_PER_BLOCK = 4
SCRATCH_BUDGET = 16 << 30
ROW_LOG_MAX = 0x7fff0000
EXTRA = {"findErrors": lambda limit: 2 * (limit + 8), "correctOverlaps": lambda limit: 0}


def _launch(log_cap, limit, extra, todo):
    """launch_size, restated: (per_wave, nwaves, blocks, scratch_bytes)."""
    per_wave = log_cap + 3 * (limit + 2) + 2 * (limit + 4) + extra + 8
    fit = max(1, SCRATCH_BUDGET // (per_wave * 4))
    nwaves = min(todo, N_CU * 8 * WAVES_PER_BLOCK, fit)
    return per_wave, nwaves, -(-nwaves // WAVES_PER_BLOCK), per_wave * nwaves * 4


@pytest.mark.parametrize("stage", sorted(EXTRA))
def test_launch_sizes(host_check, stage):
    """A launch's scratch per wave, waves, blocks and bytes for both stages' extra ints: one
    overlap, one overlap more than the grid holds, where the budget takes over from the grid, and
    the first log that the 32-bit offsets refuse."""
    extra = EXTRA[stage]
    worst = lambda l: (l + 1) ** 2 + 64                        # noqa: E731
    grid = N_CU * 8 * WAVES_PER_BLOCK
    many = 4 * grid
    budget = next(l for l in range(1, 1 << 20)
                  if SCRATCH_BUDGET // (_launch(worst(l), l, extra(l), many)[0] * 4) < grid)
    refused = next(l for l in range(46000, 1 << 20) if worst(l) > ROW_LOG_MAX)
    assert 700 < budget < 740 and worst(refused - 1) <= ROW_LOG_MAX
    cases = [(PER_ERROR * 3 + 64, 3, 1), (PER_ERROR * 3 + 64, 3, grid + 1),
             (worst(budget - 1), budget - 1, many), (worst(budget), budget, many),
             (worst(refused - 1), refused - 1, many), (worst(refused), refused, many)]
    got = _lines(host_check, "launch", N_CU, *[v for c, l, t in cases for v in (c, l, extra(l), t)])
    assert len(got) == len(cases)
    for (log_cap, limit, todo), (ok, *sized, wpb, bud) in zip(cases, got):
        assert (wpb, bud) == (WAVES_PER_BLOCK, SCRATCH_BUDGET)
        if limit == refused:
            assert ok == 0 and sized == [0, 0, 0, 0]           # refused, not sized
        else:
            assert ok == 1 and tuple(sized) == _launch(log_cap, limit, extra(limit), todo), (limit, todo)
    assert got[0][2:4] == [1, 1]                               # one overlap: one wave, one block
    assert got[1][2:4] == [grid, grid // WAVES_PER_BLOCK]      # the grid decides
    assert got[2][2] == grid and got[3][2] < grid              # then the budget does
    assert 1 <= got[4][2] < 4                                  # the largest log still gets a wave
