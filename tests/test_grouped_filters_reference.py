"""tests/grouped_filters_reference.py (the numpy reference of K8) against a plain Python loop over rows; runs without a GPU."""
import numpy as np

from tests.grouped_filters_reference import grouped_filter_counts


def test_grouped_filter_counts_match_a_loop_over_rows():
    """500 rows, 5 filters (a random one, an empty one, a full one, None, a sparse one), 7 ranges in no order: touching ones, one
    unbounded below, one unbounded above, one that no row reaches; NULL dates and dates on every bound."""
    rng = np.random.default_rng(81)
    n = 500
    ranges = [(100, 149), (150, 150), (0, 49), (151, 200), (3_000_000_000, 3_000_000_100), (60, 90), (1000, 0xFFFFFFFF)]
    bounds = [b for r in ranges if r[0] < 3_000_000_000 for b in r if b != 0xFFFFFFFF]
    dates = rng.integers(0, 260, size=n).astype(np.int64)
    dates[rng.choice(n, size=40, replace=False)] = 0
    special = np.array([1, 2000, 0xFFFFFFFF] + bounds + [b + 1 for b in bounds] + [max(b - 1, 0) for b in bounds])
    dates[rng.choice(n, size=len(special), replace=False)] = special
    dates = dates.astype(np.uint32)
    assert (dates == 0).sum() >= 40 and not ((dates >= 3_000_000_000) & (dates <= 3_000_000_100)).any()
    base = rng.random(n) < 0.8
    sparse = np.zeros(n, bool)
    sparse[rng.choice(n, size=9, replace=False)] = True
    filters = [rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool), None, sparse]
    for base_mask in (base, None):
        want = np.zeros((len(filters), len(ranges)), dtype=np.uint32)
        for row in range(n):
            if base_mask is not None and not base_mask[row]:
                continue
            date = int(dates[row])
            if date == 0:
                continue
            for r, (low, high) in enumerate(ranges):
                if low <= date <= high:
                    for f, mask in enumerate(filters):
                        if mask is None or mask[row]:
                            want[f, r] += 1
        got = grouped_filter_counts(base_mask, filters, dates, ranges)
        assert got.dtype == np.uint32 and got.shape == (5, 7)
        assert np.array_equal(got, want)
        assert not got[1].any() and not got[:, 4].any() and np.array_equal(got[2], got[3])
        assert got[2, 2] > 0 and got[2, 6] > 0 and got[2, 1] > 0 and got[4].sum() > 0
