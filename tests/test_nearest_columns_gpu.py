"""The per-row selection of NearestAmong (K14, csrc/silo_gpu_neighbours.hip) through silo_gpu_nearest_columns, on numpy cell tables
against tests/neighbours_reference.py (pinned against a full lexsort per row without a GPU by tests/test_neighbours_reference.py).

The lists are unique under the order (distance, column), so every comparison is an exact equality; the lists and the counts are
filled with 0xA5 bytes before the launch, and the entries at or past a row's count, four guard words behind each buffer included,
must still hold them.  Column counts stand around a wave, the 1 024 threads of the block (a thread's second column) and the limit.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.neighbours_reference import NOT_ELIGIBLE, nearest_columns  # noqa: E402

FILL = 0xA5
SENTINEL = 0xA5A5A5A5
GUARD = 4
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT


def _check(cells, k):
    """(lists uint32 [m][k][3], counts uint32 [m]) as the device leaves them, after the comparison with the reference."""
    from silo_amd import binding

    m, n = cells.shape[:2]
    lists, counts = binding.nearest_columns(cells, m, n, k, fill=FILL, guard_words=GUARD)
    assert len(lists) == m * k * 3 + GUARD and len(counts) == m + GUARD
    assert (lists[m * k * 3:] == SENTINEL).all() and (counts[m:] == SENTINEL).all(), "the guard words were written"
    want_lists, want_counts = nearest_columns(cells, k, untouched=SENTINEL)
    lists, counts = lists[:m * k * 3].reshape(m, k, 3), counts[:m]
    assert np.array_equal(counts, want_counts), (m, n, k, counts[:8], want_counts[:8])
    assert np.array_equal(lists, want_lists), (m, n, k, np.argwhere(lists != want_lists)[:5])
    return lists, counts


def _cells(rng, m, n, high, absent=0.0):
    cells = rng.integers(0, high, size=(m, n, 2), dtype=np.uint32)
    if absent:
        cells[rng.random((m, n)) < absent] = NOT_ELIGIBLE
    return cells


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.NEIGHBOUR_THREADS, binding.MAX_CROSS_COLUMNS, binding.MAX_CROSS_ROWS, binding.MAX_NEIGHBOUR_COLUMNS) == (1024, 8192, 2048, 64)


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1023, 1024, 1025, 4097, 8192])
def test_shapes(built, n, k):
    for m in (1, 3, 70):
        rng = np.random.default_rng(7100 + 100 * m + n + k)
        lists, counts = _check(_cells(rng, m, n, 6, absent=0.2), k)   # distances 0 .. 5: ties everywhere
        assert (counts <= min(k, n)).all()
        _check(_cells(rng, m, n, 2**20, absent=0.5), k)               # distances that hardly tie
        none, counts = _check(np.full((m, n, 2), NOT_ELIGIBLE, dtype=np.uint32), k)  # no eligible cell: nothing listed
        assert (counts == 0).all() and (none == SENTINEL).all()
        zeros = np.zeros((m, n, 2), dtype=np.uint32)
        zeros[..., 1] = np.arange(n)
        lists, counts = _check(zeros, k)                              # all at distance 0: the lowest columns
        assert (counts == min(k, n)).all() and (lists[:, :min(k, n), 0] == np.arange(min(k, n))).all()


@pytest.mark.parametrize("k", [1, 5, 64])
def test_500_columns_tied_at_the_kth_distance(built, k):
    rng = np.random.default_rng(7200 + k)
    m, n = 4, 3000
    cells = _cells(rng, m, n, 1000)
    cells[..., 0] += 10
    for row in range(m):
        cells[row, rng.choice(n, size=k - 1, replace=False), 0] = rng.integers(0, 7, size=k - 1)   # k - 1 columns below the tie
        tied = rng.choice(np.flatnonzero(cells[row, :, 0] >= 10), size=500, replace=False)
        cells[row, tied, 0] = 7
        lists, counts = _check(cells[row:row + 1], k)
        assert counts[0] == k and lists[0, k - 1].tolist()[:2] == [int(tied.min()), 7]
    _check(cells, k)


def test_fewer_than_k_eligible_cells_and_rows_that_differ(built):
    rng = np.random.default_rng(7300)
    m, n, k = 70, 1500, 64
    cells = np.full((m, n, 2), NOT_ELIGIBLE, dtype=np.uint32)
    for row in range(m):   # row r has r eligible cells: 0 .. 69 around k
        columns = rng.choice(n, size=row, replace=False)
        cells[row, columns] = rng.integers(0, 50, size=(row, 2))
    lists, counts = _check(cells, k)
    assert counts.tolist() == [min(row, k) for row in range(m)]
    assert len({lists[row, :counts[row]].tobytes() for row in range(m)}) == m  # every row lists something else
    _check(cells, 5)


def test_large_distances_and_the_same_call_twice(built):
    from silo_amd import binding

    rng = np.random.default_rng(7400)
    m, n, k = 3, 2500, 64
    cells = rng.integers(65536, 2**32 - 1, size=(m, n, 2), dtype=np.uint32)
    cells[0, :, 0] = NOT_ELIGIBLE
    cells[0, [7, 2000], 0] = [NOT_ELIGIBLE - 1, NOT_ELIGIBLE - 1]   # the largest distance there is, twice: by column
    cells[1, 100:140, 0] = NOT_ELIGIBLE - 1
    lists, counts = _check(cells, k)
    assert counts.tolist() == [2, k, k] and lists[0, :2, :2].tolist() == [[7, NOT_ELIGIBLE - 1], [2000, NOT_ELIGIBLE - 1]]
    assert lists[1:, :, 1].min() > 65535
    first = binding.nearest_columns(cells, m, n, k, fill=FILL, guard_words=GUARD)
    second = binding.nearest_columns(cells, m, n, k, fill=FILL, guard_words=GUARD)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_the_limit_of_2048_rows(built):
    rng = np.random.default_rng(7500)
    _, counts = _check(_cells(rng, 2048, 70, 5, absent=0.3), 5)
    assert (counts == 5).all()


def test_refusals_no_rows_and_no_columns(built):
    from silo_amd import binding

    lib = binding.load_library()
    rng = np.random.default_rng(7600)
    m, n, k = 5, 70, 3
    cells = _cells(rng, m, n, 4)
    cells_dev = binding.device_malloc(cells.nbytes)
    binding._check(lib.silo_gpu_memcpy_h2d(cells_dev, binding._ptr(cells), cells.nbytes, None))
    list_words = m * k * 3 + GUARD
    lists_dev = binding.device_malloc(list_words * 4, fill=FILL)
    counts_dev = binding.device_malloc((m + GUARD) * 4, fill=FILL)
    null = ctypes.c_void_p(0)
    refused = [
        lib.silo_gpu_nearest_columns(null, m, n, k, lists_dev, counts_dev, None),
        lib.silo_gpu_nearest_columns(cells_dev, m, n, k, null, counts_dev, None),
        lib.silo_gpu_nearest_columns(cells_dev, m, n, k, lists_dev, null, None),
        lib.silo_gpu_nearest_columns(cells_dev, m, n, 0, lists_dev, counts_dev, None),
        lib.silo_gpu_nearest_columns(cells_dev, m, n, binding.MAX_NEIGHBOUR_COLUMNS + 1, lists_dev, counts_dev, None),
        lib.silo_gpu_nearest_columns(cells_dev, binding.MAX_CROSS_ROWS + 1, n, k, lists_dev, counts_dev, None),
        lib.silo_gpu_nearest_columns(cells_dev, m, binding.MAX_CROSS_COLUMNS + 1, k, lists_dev, counts_dev, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_nearest_columns" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_nearest_columns(cells_dev, 0, n, k, lists_dev, counts_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (binding.device_read(lists_dev, np.uint32, list_words) == SENTINEL).all()
    assert (binding.device_read(counts_dev, np.uint32, m + GUARD) == SENTINEL).all()
    # no columns: the counts are written as 0, and nothing else
    binding._check(lib.silo_gpu_nearest_columns(cells_dev, m, 0, k, lists_dev, counts_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (binding.device_read(lists_dev, np.uint32, list_words) == SENTINEL).all()
    assert binding.device_read(counts_dev, np.uint32, m + GUARD).tolist() == [0] * m + [SENTINEL] * GUARD
    # the valid call on the same buffers
    binding._check(lib.silo_gpu_nearest_columns(cells_dev, m, n, k, lists_dev, counts_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    want_lists, want_counts = nearest_columns(cells, k)
    got = binding.device_read(lists_dev, np.uint32, list_words)
    assert np.array_equal(got[:m * k * 3].reshape(m, k, 3), want_lists) and (got[m * k * 3:] == SENTINEL).all()
    assert np.array_equal(binding.device_read(counts_dev, np.uint32, m + GUARD)[:m], want_counts)
    for pointer in (cells_dev, lists_dev, counts_dev):
        binding.device_free(pointer)
