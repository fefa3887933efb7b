"""The connected components of a bit matrix (K12, csrc/silo_gpu_clusters.hip) through silo_gpu_adjacency_components, on numpy bit
matrices against the union-find of tests/clusters_reference.py (pinned against a breadth-first search without a GPU by
tests/test_clusters_reference.py): sizes around a word of the matrix, around the 1 024 threads of the block and at the limit; no
edges, all edges, a path over a shuffled numbering, a star, two interleaved components, random sparse graphs, stray bits past n;
two identical runs; the refusals.  The labels are filled with 0xA5 bytes before the launch.  The rounds are at most n; no smaller
number is asserted (DESIGN.md §19 holds the rounds that were seen).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.clusters_reference import adjacency_words, components, pack_bits  # noqa: E402

FILL = 0xA5
SIZES = [1, 2, 63, 64, 65, 1000, 4097, 8192]
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT


def _edges_to_bits(n, first, second):
    """uint64 [n][AW] with the bits (first, second) and (second, first) set."""
    bits = np.zeros((n, adjacency_words(n)), dtype=np.uint64)
    for a, b in ((first, second), (second, first)):
        np.bitwise_or.at(bits, (a, b >> 6), np.uint64(1) << (b & 63).astype(np.uint64))
    return bits


def _run(bits, n):
    from silo_amd import binding

    labels, rounds = binding.adjacency_components(bits, n, fill=FILL)
    assert labels.dtype == np.uint32 and len(labels) == n
    assert 1 <= rounds <= n, rounds
    return labels, rounds


def test_the_sizes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert binding.COMPONENTS_THREADS == 1024 and binding.MAX_CLUSTER_ROWS == SIZES[-1]
    assert 1000 < binding.COMPONENTS_THREADS < 4097  # rows below and above one row per thread


@pytest.mark.parametrize("n", SIZES)
def test_no_edges_and_all_edges(built, n):
    labels, rounds = _run(np.zeros((n, adjacency_words(n)), dtype=np.uint64), n)
    assert np.array_equal(labels, np.arange(n)) and rounds == 1
    labels, _ = _run(pack_bits(~np.eye(n, dtype=bool)), n)
    assert not labels.any()


def test_a_path_over_a_shuffled_numbering(built):
    """2 049 rows in one path whose order is a shuffle, with row 0 in the middle of it: plain propagation would need a thousand
    rounds."""
    n = 2049
    rng = np.random.default_rng(3100)
    order = rng.permutation(np.arange(1, n))
    order = np.concatenate([order[:n // 2], [0], order[n // 2:]])
    bits = _edges_to_bits(n, order[:-1], order[1:])
    assert (np.bitwise_count(bits).sum(axis=1) <= 2).all() and np.bitwise_count(bits).sum() == 2 * (n - 1)
    labels, rounds = _run(bits, n)
    assert not labels.any()
    print(f"shuffled path of {n} rows: {rounds} rounds")
    # two paths: cut in the middle, the second half's lowest row is its label
    bits = _edges_to_bits(n, np.delete(order[:-1], n // 2), np.delete(order[1:], n // 2))
    labels, _ = _run(bits, n)
    assert np.array_equal(labels, components(bits)) and set(labels.tolist()) == {0, int(order[n // 2 + 1:].min())}


@pytest.mark.parametrize("n", [65, 1000, 8192])
def test_a_star_whose_hub_is_the_highest_row(built, n):
    hub = np.full(n - 1, n - 1)
    labels, _ = _run(_edges_to_bits(n, hub, np.arange(n - 1)), n)
    assert not labels.any()
    # without row 0 in it: the star's label is 1, row 0 stays alone
    labels, _ = _run(_edges_to_bits(n, hub[1:], np.arange(1, n - 1)), n)
    assert labels[0] == 0 and (labels[1:] == 1).all()


@pytest.mark.parametrize("n", [2, 64, 65, 1000, 4097])
def test_even_and_odd_rows_as_two_interleaved_components(built, n):
    rows = np.arange(n - 2)
    labels, _ = _run(_edges_to_bits(n, rows, rows + 2), n)
    assert np.array_equal(labels, np.arange(n) % 2)


@pytest.mark.parametrize("n,edges", [(63, 20), (65, 30), (1000, 400), (4097, 2500), (8192, 5000), (8192, 30_000)])
def test_random_sparse_graphs(built, n, edges):
    rng = np.random.default_rng(3200 + n + edges)
    first, second = rng.integers(0, n, size=(2, edges))
    keep = first != second
    first, second = first[keep], second[keep]
    bits = _edges_to_bits(n, first, second)
    want = components(bits)
    isolated = np.bitwise_count(bits).sum(axis=1) == 0
    if edges < n:
        assert isolated.sum() > n // 10
    labels, rounds = _run(bits, n)
    assert np.array_equal(labels, want)
    assert np.array_equal(labels[isolated], np.flatnonzero(isolated))
    assert 3 <= len(np.unique(want)) and np.bincount(want).max() >= 3
    print(f"random graph of {n} rows and {len(first)} edges: {rounds} rounds, {len(np.unique(want))} components")
    again, rounds_again = _run(bits, n)
    assert np.array_equal(again, labels)


@pytest.mark.parametrize("n", [1, 63, 65, 1000, 4097])
def test_stray_bits_at_or_past_n_change_nothing(built, n):
    """Every bit at or past n of every row's last word set: they name rows that do not exist and must never index the labels."""
    rng = np.random.default_rng(3300 + n)
    first, second = rng.integers(0, n, size=(2, n // 3))
    keep = first != second
    bits = _edges_to_bits(n, first[keep], second[keep])
    want, _ = _run(bits, n)
    assert np.array_equal(want, components(bits))
    assert n % 64 != 0
    stray = bits.copy()
    stray[:, -1] |= ~((np.uint64(1) << np.uint64(n % 64)) - np.uint64(1))
    assert not np.array_equal(stray, bits)
    labels, _ = _run(stray, n)
    assert np.array_equal(labels, want)


def test_refusals(built):
    """NULL buffers and 8 193 rows: SILO_GPU_ERR_INVALID_ARGUMENT and nothing written; no rows: success and nothing written; a NULL
    round count is allowed; the next valid call answers exactly."""
    from silo_amd import binding

    lib = binding.load_library()
    n = 70
    rows = np.arange(n - 2)
    bits = _edges_to_bits(n, rows, rows + 2)
    bits_dev = binding.device_malloc(bits.nbytes)
    binding._check(lib.silo_gpu_memcpy_h2d(bits_dev, bits.ctypes.data_as(ctypes.c_void_p), bits.nbytes, None))
    labels_dev = binding.device_malloc((n + 4) * 4, fill=FILL)
    rounds_dev = binding.device_malloc(4, fill=FILL)
    null = ctypes.c_void_p(0)

    def read():
        return binding.device_read(labels_dev, np.uint32, n + 4), int(binding.device_read(rounds_dev, np.uint32, 1)[0])

    refused = [
        lib.silo_gpu_adjacency_components(null, n, labels_dev, rounds_dev, None),
        lib.silo_gpu_adjacency_components(bits_dev, n, null, rounds_dev, None),
        lib.silo_gpu_adjacency_components(bits_dev, binding.MAX_CLUSTER_ROWS + 1, labels_dev, rounds_dev, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_adjacency_components" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_adjacency_components(bits_dev, 0, labels_dev, rounds_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    labels, rounds = read()
    assert (labels == 0xA5A5A5A5).all() and rounds == 0xA5A5A5A5
    binding._check(lib.silo_gpu_adjacency_components(bits_dev, n, labels_dev, null, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    labels, rounds = read()
    assert np.array_equal(labels[:n], np.arange(n) % 2) and (labels[n:] == 0xA5A5A5A5).all() and rounds == 0xA5A5A5A5
    binding._check(lib.silo_gpu_adjacency_components(bits_dev, n, labels_dev, rounds_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    labels, rounds = read()
    assert np.array_equal(labels[:n], np.arange(n) % 2) and 1 <= rounds <= n
    for pointer in (bits_dev, labels_dev, rounds_dev):
        binding.device_free(pointer)
