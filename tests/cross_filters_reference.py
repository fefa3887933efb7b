"""The numpy reference of the pair count of two filter lists (K9, silo_gpu_filters_cross) — test infrastructure only.

Pinned against a plain loop over rows by tests/test_cross_filters_reference.py and used by tests/test_cross_filters_gpu.py and
tests/test_cross_tabulation_gpu.py.
"""
import numpy as np


def _matrix(masks, n):
    """int64 [len(masks)][n]: a 0 / 1 row per mask, None = all rows."""
    out = np.ones((len(masks), n), dtype=np.int64)
    for k, mask in enumerate(masks):
        if mask is not None:
            out[k] = np.asarray(mask, dtype=bool)
    return out


def cross_filter_counts(base, row_masks, col_masks, n):
    """uint32 [len(row_masks)][len(col_masks)]: per pair the rows below n that the base, the row mask and the column mask all
    select.  Masks are bool arrays of n rows; None (the base or an entry) = all rows."""
    rows = _matrix(row_masks, n)
    if base is not None:
        rows = rows * np.asarray(base, dtype=bool).astype(np.int64)[None, :]
    return (rows @ _matrix(col_masks, n).T).astype(np.uint32).reshape(len(row_masks), len(col_masks))
