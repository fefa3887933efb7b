"""The numpy reference of the matrix of edge weights and of its minimum spanning forest (K13, silo_gpu_distance_weights /
silo_gpu_spanning_forest) — test infrastructure only.

Pinned against a plain Kruskal with a union-find and against tests/clusters_reference.py by tests/test_spanning_reference.py and
used by tests/test_distance_weights_gpu.py, tests/test_spanning_forest_gpu.py and tests/test_minimum_spanning_tree_gpu.py.
"""
import numpy as np

from tests.clusters_reference import linked_pairs, pair_counts

NO_EDGE = 0xFFFFFFFF   # a cell that is no edge; as max_distance: no bound on the distance
ROW_BITS = 13          # SILO_GPU_SPANNING_KEY_ROW_BITS
WEIGHT_SHIFT = 26      # SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT
_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def weights_of(differing, compared, max_distance, min_compared):
    """uint32 [n][n]: differing where i != j and differing <= max_distance and compared >= min_compared, NO_EDGE elsewhere."""
    return np.where(linked_pairs(differing, compared, max_distance, min_compared), differing, np.uint32(NO_EDGE)).astype(np.uint32)


def weights(chars, valid_chars, max_distance, min_compared):
    """uint32 [n][n] for chars uint8 [n][P]: what silo_gpu_distance_weights leaves."""
    return weights_of(*pair_counts(chars, valid_chars), max_distance, min_compared)


def keys_of(weight, i, j):
    """SILO_GPU_SPANNING_KEY, elementwise: weight << 26 | i << 13 | j as uint64."""
    return (np.asarray(weight, dtype=np.uint64) << np.uint64(WEIGHT_SHIFT)) | (np.asarray(i, dtype=np.uint64) << np.uint64(ROW_BITS)) | np.asarray(j, dtype=np.uint64)


def key_fields(keys):
    """(weight, i, j), int64 arrays, of uint64 keys."""
    keys = np.asarray(keys, dtype=np.uint64)
    mask = np.uint64((1 << ROW_BITS) - 1)
    return ((keys >> np.uint64(WEIGHT_SHIFT)).astype(np.int64), ((keys >> np.uint64(ROW_BITS)) & mask).astype(np.int64), (keys & mask).astype(np.int64))


def forest(matrix):
    """uint64 [edges]: the keys, ascending, of the minimum spanning forest of the symmetric matrix uint32 [n][n] (NO_EDGE: no edge,
    the diagonal is ignored) under the strict order of the keys.  Prim with a restart: per step one row lowers the best key of every
    vertex, the lowest key of a vertex outside the forest is the next edge; with none left, the lowest vertex outside starts the
    next tree."""
    matrix = np.asarray(matrix, dtype=np.uint32)
    n = len(matrix)
    index = np.arange(n, dtype=np.uint64)
    best = np.full(n, _NO_KEY, dtype=np.uint64)
    inside = np.zeros(n, dtype=bool)
    found = []
    u = 0
    for step in range(n):
        inside[u] = True
        if step == n - 1:
            break
        row = matrix[u]
        offered = keys_of(row, np.minimum(index, np.uint64(u)), np.maximum(index, np.uint64(u)))
        offered[row == NO_EDGE] = _NO_KEY
        offered[u] = _NO_KEY
        np.minimum(best, offered, out=best)
        outside = np.where(inside, _NO_KEY, best)
        v = int(np.argmin(outside))
        if outside[v] == _NO_KEY:
            u = int(np.argmin(inside))  # the lowest vertex outside
        else:
            found.append(outside[v])
            u = v
    return np.sort(np.array(found, dtype=np.uint64))


def cut(keys, n, max_distance):
    """uint32 [n]: per row the lowest row of its component in the forest `keys` without the edges heavier than max_distance."""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for weight, i, j in zip(*key_fields(keys)):
        if weight <= max_distance:
            a, b = find(int(i)), find(int(j))
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)
