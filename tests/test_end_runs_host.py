"""CPU-side checks of the host rule of the end runs of the gap symbol (layout_choice.h): which one-hot rows of '-' the Mutations
scan may count from the sequences' ends, and what is left of such a row as residual keys."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_HOT, IMPLICIT, IDENTITY = 0x40, 0x20, 0x80


@pytest.fixture(scope="module")
def rule(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "lapis-silo_amd", "lib", "libend_runs_host.so"))
    lib.end_run_covers.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.end_run_residual.argtypes = [ctypes.c_uint64] * 4
    lib.end_run_residual.restype = ctypes.c_uint64
    lib.end_runs_pay.argtypes = [ctypes.c_uint64] * 5
    return lib


def test_a_row_is_covered_only_at_a_position_that_derives_another_symbol(rule):
    cost = rule.end_run_key_cost()
    row_bytes = 1_250_000
    assert cost == 10
    assert rule.end_run_covers(ONE_HOT | IMPLICIT | 1, 2, 0, 0, row_bytes, cost) == 1
    assert rule.end_run_covers(ONE_HOT | IMPLICIT | 1, 0, 0, 0, row_bytes, cost) == 0  # '-' is the derived symbol
    assert rule.end_run_covers(ONE_HOT | 1, 2, 0, 0, row_bytes, cost) == 0            # nothing is derived: no finish step
    assert rule.end_run_covers(2, 2, 0, 0, row_bytes, cost) == 0                      # code planes
    assert rule.end_run_covers(IDENTITY | 3, 2, 0, 0, row_bytes, cost) == 0


def test_the_residual_has_to_cost_less_than_the_row(rule):
    cost, row_bytes = 10, 17_664
    layout = ONE_HOT | IMPLICIT | 2
    assert rule.end_run_covers(layout, 1, 0, 1766, row_bytes, cost) == 1  # 17 660 < 17 664
    assert rule.end_run_covers(layout, 1, 0, 1767, row_bytes, cost) == 0  # 17 670
    assert rule.end_run_covers(layout, 1, 0, 2208, row_bytes, 8) == 0     # 8 x 2 208 = the row: not cheaper
    assert rule.end_run_covers(layout, 1, 0, 2207, row_bytes, 8) == 1


def test_the_stream_has_to_cost_less_than_the_rows_it_replaces(rule):
    row_bytes = 1_250_000
    assert rule.end_runs_pay(439, row_bytes, 19_900_241, 1_976, 10) == 1  # a genome: 549 MB of rows for 199 MB of events
    assert rule.end_runs_pay(4, row_bytes, 10_200_018, 1_111, 10) == 0    # a gene: 5 MB of rows for 102 MB
    assert rule.end_runs_pay(0, row_bytes, 0, 0, 10) == 0
    assert rule.end_runs_pay(8, 1000, 799, 0, 10) == 1 and rule.end_runs_pay(8, 1000, 800, 0, 10) == 0


def test_residual_against_a_direct_count(rule):
    rng = np.random.default_rng(5)
    n, positions = 3000, 80
    sym = rng.integers(1, 5, size=(n, positions))
    lead = np.where(rng.random(n) < 0.9, rng.geometric(1 / 10, size=n), 0)
    trail = np.where(rng.random(n) < 0.9, rng.geometric(1 / 12, size=n), 0)
    column = np.arange(positions)
    sym[column[None, :] < lead[:, None]] = 0
    sym[column[None, :] >= positions - trail[:, None]] = 0
    sym[:5] = 0                                  # '-' throughout: counted once
    sym[rng.random((n, positions)) < 0.01] = 0   # interior deletions (some lengthen a run)
    sym[rng.random((n, positions)) < 0.01] = 9   # other symbols cut cells off from their run
    not_gap = sym != 0
    lead = np.where(not_gap.any(axis=1), not_gap.argmax(axis=1), positions)
    trail_start = np.where(not_gap.any(axis=1), positions - not_gap[:, ::-1].argmax(axis=1), positions)
    for p in range(positions):
        inside = (column[p] < lead) | (column[p] >= trail_start)
        direct = int(((sym[:, p] == 0) & ~inside).sum())
        got = rule.end_run_residual(int((sym[:, p] == 0).sum()), n, int((lead <= p).sum()), int((trail_start <= p).sum()))
        assert got == direct, p
