"""tests/spanning_reference.py (the numpy reference of K13) against a plain Kruskal with a union-find and against the components of
tests/clusters_reference.py, and the constants of K13 that silo_amd/binding.py restates against include/silo_gpu.h; runs without a
GPU."""
import os
import re

import numpy as np
import pytest

from tests.clusters_reference import components, linked_pairs, pair_counts
from tests.pair_distances_reference import NUC_CHARS, NUC_VALID
from tests.spanning_reference import NO_EDGE, ROW_BITS, WEIGHT_SHIFT, cut, forest, key_fields, keys_of, weights, weights_of


def _kruskal(matrix):
    """The forest by the textbook: every edge i < j by ascending key, kept if it joins two trees."""
    n = len(matrix)
    edges = sorted((int(matrix[i, j]) << WEIGHT_SHIFT | i << ROW_BITS | j) for i in range(n) for j in range(i + 1, n) if matrix[i, j] != NO_EDGE)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    kept = []
    for key in edges:
        a, b = find((key >> ROW_BITS) & 8191), find(key & 8191)
        if a != b:
            parent[a] = b
            kept.append(key)
    return np.array(kept, dtype=np.uint64)


def _symmetric(rng, n, high, absent):
    """uint32 [n][n], symmetric: weights below `high`, a share `absent` of the pairs NO_EDGE, the diagonal NO_EDGE."""
    upper = rng.integers(0, high, size=(n, n), dtype=np.uint32)
    upper[rng.random((n, n)) < absent] = NO_EDGE
    upper = np.triu(upper, 1)
    matrix = upper + upper.T
    np.fill_diagonal(matrix, NO_EDGE)
    return matrix


def _block_diagonal(rng, sizes, high, absent):
    n = sum(sizes)
    matrix = np.full((n, n), NO_EDGE, dtype=np.uint32)
    begin = 0
    for size in sizes:
        matrix[begin:begin + size, begin:begin + size] = _symmetric(rng, size, high, absent)
        begin += size
    order = rng.permutation(n)  # the components interleaved
    return matrix[np.ix_(order, order)]


def _trees(keys, n):
    return len(set(cut(keys, n, NO_EDGE).tolist()))


@pytest.mark.parametrize("n,high,absent", [(1, 5, 0.0), (2, 5, 0.0), (3, 1, 0.0), (40, 4, 0.0), (65, 3, 0.6), (150, 1000, 0.0), (300, 4, 0.995), (300, 2**32 - 1, 0.5)])
def test_forest_matches_kruskal(n, high, absent):
    rng = np.random.default_rng(400 + n + high % 7)
    matrix = _symmetric(rng, n, high, absent)
    got = forest(matrix)
    assert got.dtype == np.uint64 and np.array_equal(got, _kruskal(matrix))
    assert len(got) == n - _trees(got, n) and (np.diff(got.astype(object)) > 0).all()
    weight, i, j = key_fields(got)
    assert (i < j).all() and (j < n).all() and np.array_equal(weight, matrix[i, j].astype(np.int64))
    assert np.array_equal(keys_of(weight, i, j), got)
    if absent > 0.9:
        assert 1 < _trees(got, n) < n  # really disconnected, with trees of more than one vertex


def test_equal_weights_no_edges_and_disconnected_graphs():
    for n in (2, 9, 130):
        for value in (0, 7):
            matrix = np.full((n, n), value, dtype=np.uint32)
            np.fill_diagonal(matrix, NO_EDGE)
            want = keys_of(np.full(n - 1, value), np.zeros(n - 1), np.arange(1, n))  # the star of vertex 0
            assert np.array_equal(forest(matrix), want) and np.array_equal(_kruskal(matrix), want)
        nothing = np.full((n, n), NO_EDGE, dtype=np.uint32)
        assert len(forest(nothing)) == 0 and len(_kruskal(nothing)) == 0
    assert len(forest(np.zeros((0, 0), np.uint32))) == 0 and len(forest(np.full((1, 1), 3, np.uint32))) == 0
    rng = np.random.default_rng(410)
    for sizes, high, absent in (((1, 1, 5, 40, 1, 17), 3, 0.3), ((100, 100, 50), 6, 0.0), ((30,) * 8 + (1,) * 10, 2**20, 0.5)):
        matrix = _block_diagonal(rng, sizes, high, absent)
        got = forest(matrix)
        assert np.array_equal(got, _kruskal(matrix))
        reached = components(matrix != NO_EDGE)
        assert np.array_equal(cut(got, len(matrix), NO_EDGE), reached) and len(set(reached.tolist())) >= len(sizes) > 1
        assert len(got) == len(matrix) - len(set(reached.tolist()))
    # the diagonal is ignored
    matrix = _symmetric(rng, 20, 4, 0.2)
    with_diagonal = matrix.copy()
    np.fill_diagonal(with_diagonal, 0)
    assert np.array_equal(forest(with_diagonal), forest(matrix))


def test_cutting_the_forest_gives_the_clusters_at_every_bound():
    rng = np.random.default_rng(420)
    base = rng.choice(np.frombuffer(NUC_VALID.encode(), dtype=np.uint8), size=(12, 90))[rng.integers(0, 12, size=140)]
    redrawn = rng.random(base.shape) < 0.03
    base[redrawn] = rng.choice(np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8), size=int(redrawn.sum()))
    differing, compared = pair_counts(base, NUC_VALID)
    seen = set()
    for max_distance, min_compared in ((NO_EDGE, 0), (NO_EDGE, 80), (12, 0), (6, 78)):
        matrix = weights(base, NUC_VALID, max_distance, min_compared)
        assert np.array_equal(matrix, weights_of(differing, compared, max_distance, min_compared)) and np.array_equal(matrix, matrix.T)
        assert (matrix.diagonal() == NO_EDGE).all()
        tree = forest(matrix)
        assert np.array_equal(tree, _kruskal(matrix))
        for d in (0, 1, 2, 3, 5, 8, 12, 20, 90):
            want = components(linked_pairs(differing, compared, min(d, max_distance), min_compared))
            assert np.array_equal(cut(tree, 140, d), want), (max_distance, min_compared, d)
            seen.add(len(set(want.tolist())))
    assert len(seen) >= 5 and 1 in seen  # the bounds change the clusters
    assert weights(np.zeros((3, 0), np.uint8), NUC_VALID, NO_EDGE, 0).tolist() == [[NO_EDGE, 0, 0], [0, NO_EDGE, 0], [0, 0, NO_EDGE]]
    assert (weights(np.zeros((3, 0), np.uint8), NUC_VALID, NO_EDGE, 1) == NO_EDGE).all()


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_SPANNING_ROWS == defined("SILO_GPU_MAX_SPANNING_ROWS") == defined("SILO_GPU_MAX_CLUSTER_ROWS") == 8192
    assert binding.SPANNING_THREADS == defined("SILO_GPU_SPANNING_THREADS") == 1024
    assert binding.SPANNING_KEY_ROW_BITS == defined("SILO_GPU_SPANNING_KEY_ROW_BITS") == ROW_BITS and 1 << ROW_BITS == binding.MAX_SPANNING_ROWS
    assert binding.SPANNING_KEY_WEIGHT_SHIFT == defined("SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT") == WEIGHT_SHIFT == 2 * ROW_BITS
    assert binding.NO_EDGE == NO_EDGE == 2**32 - 1
    assert binding.spanning_key(5, 3, 8191) == int(keys_of(5, 3, 8191)) == 5 * 2**26 + 3 * 2**13 + 8191
    assert [int(field[0]) for field in binding.spanning_key_fields([binding.spanning_key(2**32 - 2, 8190, 8191)])] == [2**32 - 2, 8190, 8191]
    for name in ("silo_gpu_distance_weights", "silo_gpu_spanning_forest", "silo_gpu_distance_listed_pairs"):
        assert name in binding.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", header)
