"""The numpy reference of the nearest neighbours of a query (K11, silo_gpu_query_distances / silo_gpu_nearest_rows) — test
infrastructure only.

Pinned against character-by-character and sort-everything loops and against pair_distances by
tests/test_nearest_rows_reference.py; used by tests/test_query_distances_gpu.py, tests/test_nearest_rows_gpu.py and
tests/test_nearest_neighbours_gpu.py.
"""
import numpy as np

from tests.pair_distances_reference import NOT_VALID, code_table

NO_ROW = 0xFFFFFFFF


def query_distances(chars, query, valid_chars):
    """uint32 [n][2] for chars uint8 [n][P] and query uint8 [P]: row r = (positions where the query and row r both hold a valid
    symbol and the two differ, positions where both hold a valid symbol)."""
    chars = np.asarray(chars, dtype=np.uint8)
    query = np.asarray(query, dtype=np.uint8)
    table = code_table(valid_chars)
    both = (table[chars] != NOT_VALID) & (table[query] != NOT_VALID)[None, :]
    out = np.zeros((chars.shape[0], 2), dtype=np.uint32)
    out[:, 1] = both.sum(axis=1)
    out[:, 0] = (both & (chars != query[None, :])).sum(axis=1)
    return out


def nearest(table, mask, k, max_distance=None, exclude=None):
    """The rows (int64, ascending by (distance, row)) of the k smallest (distance, row) among the rows of table uint32 [n][2]
    (distance, compared) that `mask` selects (None = all rows), other than `exclude`, with distance <= max_distance."""
    table = np.asarray(table)
    distance = table[:, 0].astype(np.int64)
    eligible = np.ones(len(table), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    if exclude is not None and exclude != NO_ROW and exclude < len(table):
        eligible[exclude] = False
    if max_distance is not None and max_distance != NO_ROW:
        eligible &= distance <= max_distance
    rows = np.flatnonzero(eligible)
    order = np.argsort(distance[rows], kind="stable")  # rows are ascending: a stable sort keeps ties by row id
    return rows[order][:k]


def nearest_list(table, rows):
    """uint32 [len(rows)][3] = row, distance, compared: what silo_gpu_nearest_rows writes for those rows."""
    table = np.asarray(table, dtype=np.uint32)
    return np.column_stack([np.asarray(rows, dtype=np.uint32), table[rows, 0], table[rows, 1]]).astype(np.uint32).reshape(-1, 3)
