"""The numpy reference of the grouped mutation counts (oracle/dense.py: grouped_mutation_counts, row_groups) against
dense.mutation_counts under the mask And(filter, date in range) and against a loop over the rows.  No GPU: this keeps the
reference of tests/test_grouped_kernels_gpu.py independent of the kernels it judges."""
import numpy as np
import pytest

from oracle import dense


def _loop_reference(sym, mask, dates, ranges, cells, scan_symbols):
    groups = [dense.NO_GROUP] * len(mask)
    table = [[[0, 0] for _ in ranges] for _ in cells]
    for row in range(len(mask)):
        date = int(dates[row])
        if not mask[row] or date == 0:
            continue
        for g, (low, high) in enumerate(ranges):
            if low <= date <= high:
                groups[row] = g
                for m, (position, symbol) in enumerate(cells):
                    here = int(sym[row, position])
                    table[m][g][0] += here == symbol
                    table[m][g][1] += here in scan_symbols
    return np.array(groups, dtype=np.uint16), np.array(table, dtype=np.uint32).reshape(len(cells), len(ranges), 2)


@pytest.mark.parametrize("alphabet,n", [("nuc", 1), ("nuc", 257), ("aa", 300)])
def test_grouped_reference_matches_mutation_counts_and_a_row_loop(alphabet, n):
    rng = np.random.default_rng(5 * n + len(alphabet))
    table_size, scan_symbols = (16, [0, 1, 2, 3, 4]) if alphabet == "nuc" else (25, list(range(21)) + [23])
    positions = 6
    sym = rng.integers(0, table_size, size=(n, positions)).astype(np.uint8)
    mask = rng.random(n) < 0.7
    # touching ranges, a single day, the unbounded encodings at both ends, a range no date reaches, [0, 0]; request order mixed
    ranges = [(20, 29), (0, 9), (30, 30), (10, 19), (31, 40), (1000, 0xFFFFFFFF), (500, 600), (0, 0)][: 8 if n > 1 else 3]
    dates = rng.integers(0, 45, size=n).astype(np.uint32)
    dates[rng.random(n) < 0.1] = 0
    dates[rng.random(n) < 0.05] = 0xFFFFFFFF
    dates[rng.random(n) < 0.05] = 1000
    cells = [(p, s) for p in range(positions) for s in scan_symbols[:4]] + [(2, scan_symbols[-1]), (0, scan_symbols[0])]
    got = dense.grouped_mutation_counts(sym, mask, dates, ranges, cells, scan_symbols)
    groups = dense.row_groups(mask, dates, ranges)
    assert got.shape == (len(cells), len(ranges), 2) and got.dtype == np.uint32
    assert groups.shape == (n,) and groups.dtype == np.uint16
    for g, (low, high) in enumerate(ranges):
        in_range = (dates != 0) & (dates.astype(np.int64) >= low) & (dates.astype(np.int64) <= high)
        counts = dense.mutation_counts(sym, mask & in_range, scan_symbols)
        assert np.array_equal(groups == g, mask & in_range)
        for m, (p, s) in enumerate(cells):
            assert got[m, g, 0] == counts[p][scan_symbols.index(s)], (m, g)
            assert got[m, g, 1] == counts[p].sum(), (m, g)
    loop_groups, loop_table = _loop_reference(sym, mask, dates, ranges, cells, scan_symbols)
    assert np.array_equal(groups, loop_groups)
    assert np.array_equal(got, loop_table)
    if n > 1:
        assert got[:, :, 0].any() and (groups == dense.NO_GROUP).any() and (got[:, 6] == 0).all() and (got[:, 7] == 0).all()
        assert got[:, 5, 1].any()  # the range up to 0xFFFFFFFF holds the dates 1000 and 0xFFFFFFFF


def test_row_groups_leave_out_null_dates_and_unselected_rows():
    dates = np.array([0, 1, 5, 6, 0xFFFFFFFF, 3, 3], dtype=np.uint32)
    mask = np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool)
    assert dense.row_groups(mask, dates, [(0, 0xFFFFFFFF)]).tolist() == [0xFFFF, 0, 0, 0, 0, 0xFFFF, 0]
    assert dense.row_groups(mask, dates, [(6, 6), (0, 0), (1, 5)]).tolist() == [0xFFFF, 2, 2, 0, 0xFFFF, 0xFFFF, 2]
    assert dense.row_groups(mask, dates, []).tolist() == [0xFFFF] * 7
