"""The numpy reference of the rectangle of distances and of the k lowest columns of every row (K14, silo_gpu_distance_cross /
silo_gpu_nearest_columns) — test infrastructure only.

Pinned against a plain character double loop, the off-diagonal block of tests/clusters_reference.py and a full lexsort per row by
tests/test_neighbours_reference.py and used by tests/test_distance_cross_gpu.py, tests/test_nearest_columns_gpu.py and
tests/test_nearest_among_gpu.py.
"""
import numpy as np

from tests.pair_distances_reference import pack_planes

NOT_ELIGIBLE = 0xFFFFFFFF  # both words of a cell that is not eligible; as a self column: none; as max_distance: no bound
COLUMN_BITS = 13           # SILO_GPU_NEIGHBOUR_KEY_COLUMN_BITS: a key is distance << 13 | column
MAX_ROWS = 2048            # SILO_GPU_MAX_CROSS_ROWS
MAX_COLUMNS = 8192         # SILO_GPU_MAX_CROSS_COLUMNS
MAX_NEIGHBOURS = 64        # SILO_GPU_MAX_NEIGHBOUR_COLUMNS


def cross_counts(chars_a, chars_b, valid_chars, max_elements=1 << 22):
    """(differing, compared), uint32 [m][n] each, for chars_a uint8 [m][P] against chars_b uint8 [n][P], from the words of
    pack_planes with np.bitwise_count: what silo_gpu_distance_pairs counts for a pair, for the whole rectangle.  Rows of the first
    side are taken in chunks of at most max_elements / (n words) rows."""
    chars_a = np.asarray(chars_a, dtype=np.uint8)
    chars_b = np.asarray(chars_b, dtype=np.uint8)
    m, positions = chars_a.shape
    n = chars_b.shape[0]
    assert chars_b.shape[1] == positions
    differing = np.zeros((m, n), dtype=np.uint32)
    compared = np.zeros((m, n), dtype=np.uint32)
    if m == 0 or n == 0 or positions == 0:
        return differing, compared
    rows = pack_planes(chars_a, valid_chars)
    columns = pack_planes(chars_b, valid_chars)
    step = max(1, max_elements // (n * rows.shape[2]))
    for begin in range(0, m, step):
        mine = rows[begin:begin + step]
        both = mine[:, None, 0, :] & columns[None, :, 0, :]
        unequal = np.zeros_like(both)
        for k in range(1, rows.shape[1]):
            unequal |= mine[:, None, k, :] ^ columns[None, :, k, :]
        compared[begin:begin + step] = np.bitwise_count(both).sum(axis=-1, dtype=np.uint32)
        differing[begin:begin + step] = np.bitwise_count(both & unequal).sum(axis=-1, dtype=np.uint32)
    return differing, compared


def cells_of(differing, compared, self_columns, max_distance, min_compared):
    """uint32 [m][n][2]: what silo_gpu_distance_cross leaves — (differing, compared) where the column is eligible for the row (not
    self_columns[row], differing <= max_distance, compared >= min_compared), (NOT_ELIGIBLE, NOT_ELIGIBLE) where it is not.
    self_columns: None, or m values of which those at or past n name no column."""
    differing = np.asarray(differing, dtype=np.uint32)
    compared = np.asarray(compared, dtype=np.uint32)
    m, n = differing.shape
    eligible = (differing.astype(np.uint64) <= max_distance) & (compared.astype(np.uint64) >= min_compared)
    if self_columns is not None:
        self_columns = np.asarray(self_columns, dtype=np.uint64)
        assert self_columns.shape == (m,)
        named = self_columns < n
        eligible[np.flatnonzero(named), self_columns[named].astype(np.int64)] = False
    cells = np.full((m, n, 2), NOT_ELIGIBLE, dtype=np.uint32)
    cells[..., 0][eligible] = differing[eligible]
    cells[..., 1][eligible] = compared[eligible]
    return cells


def nearest_columns(cells, k, untouched=NOT_ELIGIBLE):
    """(lists uint32 [m][k][3], counts uint32 [m]) for cells uint32 [m][n][2]: what silo_gpu_nearest_columns leaves — counts[i] =
    min(k, eligible cells of row i), lists[i, r] = (column, distance, compared) for r < counts[i], ascending by (distance, column);
    every entry at or past a row's count holds `untouched`.  A cell is eligible unless its first word is NOT_ELIGIBLE.  By the keys
    distance << 13 | column, as the kernel orders them."""
    cells = np.asarray(cells, dtype=np.uint32)
    m, n = cells.shape[:2]
    assert cells.shape == (m, n, 2) and 1 <= k and n <= 1 << COLUMN_BITS
    lists = np.full((m, k, 3), untouched, dtype=np.uint32)
    counts = np.zeros(m, dtype=np.uint32)
    column_mask = np.uint64((1 << COLUMN_BITS) - 1)
    for i in range(m):
        columns = np.flatnonzero(cells[i, :, 0] != NOT_ELIGIBLE)
        keys = np.sort((cells[i, columns, 0].astype(np.uint64) << np.uint64(COLUMN_BITS)) | columns.astype(np.uint64))[:k]
        counts[i] = len(keys)
        taken = (keys & column_mask).astype(np.int64)
        lists[i, :len(keys), 0] = taken
        lists[i, :len(keys), 1] = keys >> np.uint64(COLUMN_BITS)
        lists[i, :len(keys), 2] = cells[i, taken, 1]
    return lists, counts


def nearest_among(chars_a, chars_b, valid_chars, self_columns, k, max_distance=NOT_ELIGIBLE, min_compared=0):
    """The two steps in a row, for the characters of the subjects and of the candidates: (lists, counts) of nearest_columns."""
    return nearest_columns(cells_of(*cross_counts(chars_a, chars_b, valid_chars), self_columns, max_distance, min_compared), k)
