"""The numpy reference of the grouped filter count (K8, silo_gpu_filters_grouped) — test infrastructure only.

Built on oracle/dense.py's row_groups; pinned against a plain loop over rows by tests/test_grouped_filters_reference.py and used
by tests/test_grouped_filters_gpu.py.
"""
import numpy as np

from oracle import dense


def grouped_filter_counts(base, filters, dates, ranges):
    """uint32 [len(filters)][len(ranges)]: per filter (a bool mask over the rows; None = all rows) and range (inclusive (from, to)
    pairs, pairwise disjoint, in request order) the rows of base & filter whose date lies in the range; NULL dates (0) lie in
    none.  base: a bool mask, None = all rows."""
    n = len(dates)
    base = np.ones(n, bool) if base is None else np.asarray(base, dtype=bool)
    n_ranges = len(ranges)
    # row_groups(base & f) = row_groups(base) where f holds, NO_GROUP elsewhere: the ranges are gone through once for all filters
    groups = dense.row_groups(base, dates, ranges)
    grouped = groups != dense.NO_GROUP
    out = np.zeros((len(filters), n_ranges), dtype=np.uint32)
    for f, mask in enumerate(filters):
        selected = grouped if mask is None else grouped & np.asarray(mask, dtype=bool)
        out[f] = np.bincount(groups[selected], minlength=n_ranges)[:n_ranges]
    return out
