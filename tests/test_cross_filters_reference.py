"""tests/cross_filters_reference.py (the numpy reference of K9) against a plain Python loop over rows, and the constants of K9 that
silo_amd/binding.py restates against include/silo_gpu.h; runs without a GPU."""
import os
import re

import numpy as np

from tests.cross_filters_reference import cross_filter_counts


def test_cross_filter_counts_match_a_loop_over_rows():
    """300 rows; 5 row masks and 4 column masks of random densities with None, an empty and a full entry on each side; with a base
    and without one."""
    rng = np.random.default_rng(91)
    n = 300
    sparse = np.zeros(n, bool)
    sparse[rng.choice(n, size=7, replace=False)] = True
    row_masks = [rng.random(n) < 0.5, np.zeros(n, bool), None, np.ones(n, bool), sparse]
    col_masks = [None, rng.random(n) < 0.2, np.ones(n, bool), np.zeros(n, bool)]
    base = rng.random(n) < 0.7
    for base_mask in (base, None):
        want = np.zeros((len(row_masks), len(col_masks)), dtype=np.uint32)
        for row in range(n):
            if base_mask is not None and not base_mask[row]:
                continue
            for i, a in enumerate(row_masks):
                if a is not None and not a[row]:
                    continue
                for j, b in enumerate(col_masks):
                    if b is None or b[row]:
                        want[i, j] += 1
        got = cross_filter_counts(base_mask, row_masks, col_masks, n)
        assert got.dtype == np.uint32 and got.shape == (5, 4)
        assert np.array_equal(got, want)
        assert not got[1].any() and not got[:, 3].any() and np.array_equal(got[2], got[3]) and np.array_equal(got[:, 0], got[:, 2])
        assert got[2, 0] == (n if base_mask is None else base_mask.sum()) and 0 < got[4, 0] <= 7 and 0 < got[0, 1] < got[0, 0]
    assert cross_filter_counts(None, [], col_masks, n).shape == (0, 4) and cross_filter_counts(base, row_masks, [], n).shape == (5, 0)
    # the same list on both sides: symmetric, the diagonal holds the cardinalities under the base
    square = cross_filter_counts(base, row_masks, row_masks, n)
    assert np.array_equal(square, square.T)
    assert square.diagonal().tolist() == [int((base & (np.ones(n, bool) if m is None else m)).sum()) for m in row_masks]


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_CROSS_FILTERS == defined("SILO_GPU_MAX_CROSS_FILTERS") == 1024
    assert binding.CROSS_TILE == defined("SILO_GPU_CROSS_TILE")
    assert binding.CROSS_CHUNK_WORDS == defined("SILO_GPU_CROSS_CHUNK_WORDS")
    assert binding.filters_cross_scratch_bytes(3, 1024) == (3 + 1024) * 16 + 1024
