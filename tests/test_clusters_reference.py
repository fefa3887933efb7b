"""tests/clusters_reference.py (the numpy reference of K12) against tests/pair_distances_reference.py, a plain character double
loop and a breadth-first search, and the constants of K12 that silo_amd/binding.py restates against include/silo_gpu.h; runs without
a GPU."""
import os
import re
from collections import deque

import numpy as np
import pytest

from tests.clusters_reference import (NO_BOUND, adjacency_words, cluster_sizes, components, has_chain, linked_pairs, pack_bits,
                                      pair_counts, unpack_bits, within_adjacency)
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID, pair_distances

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}


def _draw(rng, name, n, positions, changed):
    all_chars, valid_chars = ALPHABETS[name]
    base = rng.choice(np.frombuffer(valid_chars.encode(), dtype=np.uint8), size=positions)
    chars = np.tile(base, (n, 1))
    redrawn = rng.random((n, positions)) < changed
    chars[redrawn] = rng.choice(np.frombuffer(all_chars.encode(), dtype=np.uint8), size=int(redrawn.sum()))
    return chars


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_within_adjacency_matches_pair_distances_and_a_double_loop(name):
    """70 rows (two words per row of the matrix) of 75 characters, in one chunk and in chunks of a few rows."""
    valid_chars = ALPHABETS[name][1]
    rng = np.random.default_rng(201)
    chars = _draw(rng, name, 70, 75, 0.05)
    table = pair_distances(chars, valid_chars)
    for max_elements in (1 << 22, 3 * 70 * 2):
        differing, compared = pair_counts(chars, valid_chars, max_elements)
        assert np.array_equal(differing, table[:, :, 0]) and np.array_equal(compared, table[:, :, 1])
    distances = np.sort(table[:, :, 0][np.triu_indices(70, 1)])
    middle = int(distances[len(distances) // 2])
    fewest = int(np.sort(table[:, :, 1][np.triu_indices(70, 1)])[len(distances) // 2])
    assert distances[0] <= middle < distances[-1]
    seen = set()
    for max_distance, min_compared in ((0, 0), (middle, 0), (middle, fewest), (NO_BOUND, fewest), (NO_BOUND, 0), (middle, NO_BOUND)):
        got = within_adjacency(chars, valid_chars, max_distance, min_compared)
        assert got.dtype == np.uint64 and got.shape == (70, 2)
        for i in range(70):
            for j in range(70):
                both = [(a, b) for a, b in zip(chars[i], chars[j]) if chr(a) in valid_chars and chr(b) in valid_chars]
                want = i != j and sum(a != b for a, b in both) <= max_distance and len(both) >= min_compared
                assert bool((int(got[i, j >> 6]) >> (j & 63)) & 1) == want
        assert not (got[:, 1] >> np.uint64(70 - 64)).any()  # bits at or past n
        seen.add(int(np.bitwise_count(got).sum()))
    assert len(seen) >= 5 and 70 * 69 in seen and 0 in seen  # the bounds change the answer
    assert within_adjacency(np.zeros((0, 5), np.uint8), valid_chars, 0, 0).shape == (0, 0)
    assert np.array_equal(unpack_bits(within_adjacency(np.zeros((3, 0), np.uint8), valid_chars, 0, 0), 3), ~np.eye(3, dtype=bool))
    assert not within_adjacency(np.zeros((3, 0), np.uint8), valid_chars, 0, 1).any()


def _bfs_labels(linked):
    n = len(linked)
    labels = np.full(n, -1, dtype=np.int64)
    for start in range(n):
        if labels[start] >= 0:
            continue
        labels[start] = start
        queue = deque([start])
        while queue:
            i = queue.popleft()
            for j in np.flatnonzero(linked[i]):
                if labels[j] < 0:
                    labels[j] = start
                    queue.append(j)
    return labels.astype(np.uint32)


@pytest.mark.parametrize("n,density", [(1, 0.0), (2, 1.0), (9, 0.2), (64, 0.02), (65, 0.03), (150, 0.008), (150, 0.0)])
def test_components_match_a_breadth_first_search(n, density):
    rng = np.random.default_rng(300 + n)
    for _ in range(4):
        upper = np.triu(rng.random((n, n)) < density, 1)
        linked = upper | upper.T
        order = rng.permutation(n)  # so that a component's lowest row is not where the search starts in the shuffled graph
        linked = linked[np.ix_(order, order)]
        bits = pack_bits(linked)
        assert np.array_equal(unpack_bits(bits, n), linked)
        want = _bfs_labels(linked)
        assert np.array_equal(components(bits), want) and np.array_equal(components(linked), want)
        sizes = cluster_sizes(want)
        assert sizes.sum() == sum(int(s) ** 2 for s in np.bincount(want) if s)
    if n == 150 and density > 0:
        assert 3 < len(set(want.tolist())) < n and sizes.max() >= 3 and has_chain(linked, want)


def test_a_path_is_a_chain_and_a_clique_is_not():
    path = np.zeros((5, 5), dtype=bool)
    for i in range(4):
        path[i, i + 1] = path[i + 1, i] = True
    assert components(path).tolist() == [0] * 5 and has_chain(path, components(path))
    clique = ~np.eye(4, dtype=bool)
    assert components(clique).tolist() == [0] * 4 and not has_chain(clique, components(clique))
    assert linked_pairs(np.zeros((2, 2), np.uint32), np.zeros((2, 2), np.uint32), 0, 0).tolist() == [[False, True], [True, False]]


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_CLUSTER_ROWS == defined("SILO_GPU_MAX_CLUSTER_ROWS") == 8192
    assert binding.MAX_DISTANCE_ROWS == defined("SILO_GPU_MAX_DISTANCE_ROWS") == 2048  # DistanceMatrix keeps its own limit
    assert binding.WITHIN_TILE_ROWS == defined("SILO_GPU_WITHIN_TILE_ROWS")
    assert binding.WITHIN_TILE_COLS == defined("SILO_GPU_WITHIN_TILE_COLS") == 64
    assert binding.WITHIN_CHUNK_WORDS == defined("SILO_GPU_WITHIN_CHUNK_WORDS")
    assert binding.COMPONENTS_THREADS == defined("SILO_GPU_COMPONENTS_THREADS")
    assert [binding.adjacency_words(n) for n in (0, 1, 64, 65, 8192)] == [adjacency_words(n) for n in (0, 1, 64, 65, 8192)] == [0, 1, 1, 2, 128]
    assert "silo_gpu_distance_within" in binding.EXPORTED_SYMBOLS and "silo_gpu_adjacency_components" in binding.EXPORTED_SYMBOLS
