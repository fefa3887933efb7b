"""The one-block forest kernel of MinimumSpanningTree (K13, csrc/silo_gpu_spanning.hip) through silo_gpu_spanning_forest, on numpy
matrices against the Prim of tests/spanning_reference.py (pinned against a Kruskal without a GPU by
tests/test_spanning_reference.py), and the listed-pairs kernel (csrc/silo_gpu_distance.hip) through
silo_gpu_distance_listed_pairs against tests/pair_distances_reference.py.

The forest is unique under the order of the keys, so every comparison is an exact equality of the keys; the edge buffer and the
count are filled with 0xA5 bytes before the launch, and the entries at or past the count, four guard entries included, must still
hold them.  Row counts stand around a wave, the 1 024 threads of the block (a thread's second vertex), the 2 048 and 4 096 keys at
which the sort pads to the next power of two, and the limit.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID, pair_distances  # noqa: E402
from tests.spanning_reference import NO_EDGE, cut, forest, key_fields, keys_of, weights  # noqa: E402

FILL = 0xA5
SENTINEL = 0xA5A5A5A5A5A5A5A5
SENTINEL32 = 0xA5A5A5A5
GUARD = 4
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}


def _check(matrix, want=None):
    """The keys the device finds for the matrix uint32 [n][n], after the comparison with the reference."""
    from silo_amd import binding

    n = len(matrix)
    want = forest(matrix) if want is None else want
    edges, count = binding.spanning_forest(matrix, n, fill=FILL, guard_words=GUARD)
    assert int(count[0]) == len(want), (n, int(count[0]), len(want))
    assert np.array_equal(edges[:len(want)], want), n
    assert (edges[len(want):] == SENTINEL).all(), "entries at or past the count were written"
    return edges[:len(want)]


def _constant(n, value):
    matrix = np.full((n, n), value, dtype=np.uint32)
    np.fill_diagonal(matrix, NO_EDGE)
    return matrix


def _symmetric(rng, n, high, absent=0.0):
    upper = rng.integers(0, high, size=(n, n), dtype=np.uint32)
    if absent:
        upper[rng.random((n, n)) < absent] = NO_EDGE
    upper = np.triu(upper, 1)
    matrix = upper + upper.T
    np.fill_diagonal(matrix, NO_EDGE)
    return matrix


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1023, 1024, 1025, 2049, 4097])
def test_no_edges_equal_weights_and_ties_everywhere(built, n):
    assert len(_check(_constant(n, NO_EDGE))) == 0
    for value in (0, 7):  # all weights equal: the star of vertex 0
        star = keys_of(np.full(n - 1, value), np.zeros(n - 1), np.arange(1, n)) if n > 1 else np.zeros(0, np.uint64)
        _check(_constant(n, value), want=star)
    rng = np.random.default_rng(4100 + n)
    got = _check(_symmetric(rng, n, 4))  # weights 0 .. 3: ties everywhere
    assert len(got) == n - 1
    sparse = _check(_symmetric(rng, n, 4, absent=1.0 - 3.0 / max(n, 4)))  # about three edges per vertex: every weight is needed
    if n > 64:
        assert len(np.unique(key_fields(sparse)[0])) == 4


def test_a_path_over_a_shuffled_numbering_with_vertex_0_in_the_middle(built):
    rng = np.random.default_rng(4200)
    n = 1500
    order = rng.permutation(n)
    order[[int(np.flatnonzero(order == 0)[0]), n // 2]] = order[[n // 2, int(np.flatnonzero(order == 0)[0])]]
    assert order[n // 2] == 0
    matrix = np.full((n, n), NO_EDGE, dtype=np.uint32)
    steps = rng.integers(0, 5, size=n - 1, dtype=np.uint32)
    matrix[order[:-1], order[1:]] = steps
    matrix[order[1:], order[:-1]] = steps
    got = _check(matrix)
    weight, i, j = key_fields(got)
    assert len(got) == n - 1 and np.array_equal(np.sort(weight), np.sort(steps.astype(np.int64)))


def test_two_interleaved_components_and_a_sparse_graph_with_isolated_vertices(built):
    rng = np.random.default_rng(4300)
    n = 1301
    matrix = _symmetric(rng, n, 6)
    parity = np.arange(n) % 2
    matrix[parity[:, None] != parity[None, :]] = NO_EDGE  # even and odd vertices never meet
    got = _check(matrix)
    labels = cut(got, n, NO_EDGE)
    assert len(got) == n - 2 and set(labels.tolist()) == {0, 1} and np.array_equal(labels, parity)
    sparse = _symmetric(rng, 2100, 50, absent=0.9995)  # about one edge per vertex: many trees, many vertices alone
    got = _check(sparse)
    alone = int(((sparse != NO_EDGE).sum(axis=1) == 0).sum())
    assert alone > 100 and 0 < len(got) < 2100 - alone


def test_large_weights_and_the_same_call_twice(built):
    rng = np.random.default_rng(4400)
    matrix = _symmetric(rng, 700, 2**32 - 1, absent=0.3)
    matrix[5, 9] = matrix[9, 5] = NO_EDGE - 1
    matrix[5, :5] = matrix[:5, 5] = NO_EDGE
    matrix[5, 6:9] = matrix[6:9, 5] = NO_EDGE
    matrix[5, 10:] = matrix[10:, 5] = NO_EDGE  # the heaviest possible edge is vertex 5's only one: it is in the forest
    first = _check(matrix)
    assert int(first[-1]) == (2**32 - 2) << 26 | 5 << 13 | 9
    assert np.array_equal(_check(matrix), first)


def test_the_limit_of_8192_rows(built):
    rng = np.random.default_rng(4500)
    got = _check(_symmetric(rng, 8192, 40))
    assert len(got) == 8191


def test_refusals_and_no_rows(built):
    from silo_amd import binding

    lib = binding.load_library()
    matrix = _constant(70, 3)
    weights_dev = binding.device_malloc(matrix.nbytes)
    binding._check(lib.silo_gpu_memcpy_h2d(weights_dev, binding._ptr(matrix), matrix.nbytes, None))
    edges_dev = binding.device_malloc((69 + GUARD) * 8, fill=FILL)
    count_dev = binding.device_malloc(4, fill=FILL)
    null = ctypes.c_void_p(0)
    refused = [
        lib.silo_gpu_spanning_forest(weights_dev, binding.MAX_SPANNING_ROWS + 1, edges_dev, count_dev, None),
        lib.silo_gpu_spanning_forest(null, 70, edges_dev, count_dev, None),
        lib.silo_gpu_spanning_forest(weights_dev, 70, null, count_dev, None),
        lib.silo_gpu_spanning_forest(weights_dev, 70, edges_dev, null, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_spanning_forest" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_spanning_forest(weights_dev, 0, edges_dev, count_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (binding.device_read(edges_dev, np.uint64, 69 + GUARD) == SENTINEL).all()
    assert int(binding.device_read(count_dev, np.uint32, 1)[0]) == SENTINEL32
    # the valid call on the same buffers
    binding._check(lib.silo_gpu_spanning_forest(weights_dev, 70, edges_dev, count_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    got = binding.device_read(edges_dev, np.uint64, 69 + GUARD)
    assert int(binding.device_read(count_dev, np.uint32, 1)[0]) == 69
    assert np.array_equal(got[:69], keys_of(np.full(69, 3), np.zeros(69), np.arange(1, 70))) and (got[69:] == SENTINEL).all()
    for pointer in (weights_dev, edges_dev, count_dev):
        binding.device_free(pointer)


# ---- silo_gpu_distance_listed_pairs ----------------------------------------------------------------------------------------------
def _draw(rng, name, n, positions, changed=0.1):
    all_chars, valid_chars = ALPHABETS[name]
    base = rng.choice(np.frombuffer(valid_chars.encode(), dtype=np.uint8), size=positions)
    chars = np.tile(base, (n, 1))
    redrawn = rng.random((n, positions)) < changed
    chars[redrawn] = rng.choice(np.frombuffer(all_chars.encode(), dtype=np.uint8), size=int(redrawn.sum()))
    return chars


@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("positions", [1, 64, 130, 4103])
def test_listed_pairs_of_the_forests_own_keys(built, name, positions):
    from silo_amd import binding

    for n in (2, 65, 300):
        rng = np.random.default_rng(4600 + n + positions)
        chars = _draw(rng, name, n, positions, changed=0.05 if positions > 100 else 0.4)
        table = pair_distances(chars, ALPHABETS[name][1])  # uint32 [n][n][2]: (differing, compared)
        keys = forest(weights(chars, ALPHABETS[name][1], NO_EDGE, 0))
        assert len(keys) == n - 1
        weight, i, j = key_fields(keys)
        planes = binding.distance_pack_rows(name, chars, fill=FILL)
        try:
            got = binding.distance_listed_pairs(name, planes, n, positions, keys, len(keys), n - 1, fill=FILL, guard_words=GUARD)
            assert np.array_equal(got[:n - 1], table[np.minimum(i, j), np.maximum(i, j)]) and np.array_equal(got[:n - 1, 0], weight)
            assert (got[n - 1:] == SENTINEL32).all()
            if n == 300:
                # a count of 0; max_pairs below the count; a count below max_pairs; a key that names a row >= n
                assert (binding.distance_listed_pairs(name, planes, n, positions, keys, 0, n - 1, fill=FILL) == SENTINEL32).all()
                few = binding.distance_listed_pairs(name, planes, n, positions, keys, len(keys), 7, fill=FILL, guard_words=GUARD)
                assert np.array_equal(few[:7], got[:7]) and (few[7:] == SENTINEL32).all()
                some = binding.distance_listed_pairs(name, planes, n, positions, keys, 9, n - 1, fill=FILL)
                assert np.array_equal(some[:9], got[:9]) and (some[9:] == SENTINEL32).all()
                stray = keys.copy()
                stray[3] = keys_of(1, 5, n)
                stray[4] = keys_of(0, n + 7, 8191)
                out = binding.distance_listed_pairs(name, planes, n, positions, stray, len(stray), n - 1, fill=FILL)
                assert (out[3:5] == NO_EDGE).all() and np.array_equal(out[:3], got[:3]) and np.array_equal(out[5:], got[5:n - 1])
        finally:
            binding.device_free(planes)


def test_listed_pairs_refusals(built):
    from silo_amd import binding

    lib = binding.load_library()
    rng = np.random.default_rng(4700)
    chars = _draw(rng, "nuc", 70, 70)
    planes_dev = binding.distance_pack_rows("nuc", chars)
    keys = forest(weights(chars, NUC_VALID, NO_EDGE, 0))
    edges_dev = binding.device_malloc(keys.nbytes)
    binding._check(lib.silo_gpu_memcpy_h2d(edges_dev, binding._ptr(keys), keys.nbytes, None))
    count = np.array([len(keys)], dtype=np.uint32)
    count_dev = binding.device_malloc(4)
    binding._check(lib.silo_gpu_memcpy_h2d(count_dev, binding._ptr(count), 4, None))
    out_dev = binding.device_malloc(69 * 8, fill=FILL)
    null = ctypes.c_void_p(0)
    refused = [
        lib.silo_gpu_distance_listed_pairs(0, planes_dev, binding.MAX_SPANNING_ROWS + 1, 70, edges_dev, count_dev, 69, out_dev, None),
        lib.silo_gpu_distance_listed_pairs(2, planes_dev, 70, 70, edges_dev, count_dev, 69, out_dev, None),
        lib.silo_gpu_distance_listed_pairs(0, null, 70, 70, edges_dev, count_dev, 69, out_dev, None),
        lib.silo_gpu_distance_listed_pairs(0, planes_dev, 70, 70, null, count_dev, 69, out_dev, None),
        lib.silo_gpu_distance_listed_pairs(0, planes_dev, 70, 70, edges_dev, null, 69, out_dev, None),
        lib.silo_gpu_distance_listed_pairs(0, planes_dev, 70, 70, edges_dev, count_dev, 69, null, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_distance_listed_pairs" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_distance_listed_pairs(0, planes_dev, 70, 70, edges_dev, count_dev, 0, out_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (binding.device_read(out_dev, np.uint32, 69 * 2) == SENTINEL32).all()
    binding._check(lib.silo_gpu_distance_listed_pairs(0, planes_dev, 70, 70, edges_dev, count_dev, 69, out_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    weight, i, j = key_fields(keys)
    assert np.array_equal(binding.device_read(out_dev, np.uint32, 69 * 2).reshape(69, 2), pair_distances(chars, NUC_VALID)[i, j])
    for pointer in (planes_dev, edges_dev, count_dev, out_dev):
        binding.device_free(pointer)
