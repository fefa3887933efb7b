"""The pair count of two filter lists (K9, csrc/silo_gpu_cross.hip) through silo_gpu_filters_cross, against the numpy reference of
tests/cross_filters_reference.py (pinned without a GPU by tests/test_cross_filters_reference.py).

tests/test_cross_tabulation_gpu.py reaches K9 through JSON and the engine.  Here the entry point gets the shapes where its kernel
takes another path: row counts around a word, the 2 048-row padding and a block of 256 words; filters per side around the tile of
8 x 8 and at the limit of 1 024; bitsets and a base with their padding bits set; NULL entries and a NULL base; the same array on
both sides; cells that several blocks add to; index arrays that permute, scatter and fill sub-blocks; the refusals of the entry.
Every comparison is an exact integer equality.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402
from tests.cross_filters_reference import cross_filter_counts  # noqa: E402
from tests.test_grouped_filters_gpu import _one_position_store, _random_masks, _upload_filters  # noqa: E402

N_MID = 2_049     # two lines of row words: what the cases around the tile and at the limit run on
N_BIG = 140_003   # three chunks of row words, the last one partial


def _cross(store, base_ptr, row_ptrs, col_ptrs, **options):
    return store.filters_cross(base_ptr, row_ptrs, col_ptrs, **options)


# ---- a: row counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 16_385])
def test_row_counts_and_padding_bits(built, n):
    """3 x 4 filters at row counts around a word, the 2 048-row padding and a block of 256 words; the filters of both sides and the
    base have every padding bit set: rows past sequence_count never count, and NULL x NULL under a NULL base is sequence_count."""
    rng = np.random.default_rng(900 + n)
    row_masks = [rng.random(n) < 0.5, np.ones(n, bool), rng.random(n) < 0.1]
    col_masks = [np.ones(n, bool), rng.random(n) < 0.6, rng.random(n) < 0.3, rng.random(n) < 0.9]
    base = rng.random(n) < 0.8
    with _one_position_store(n) as store:
        padded_rows = store.row_words * 64
        assert padded_rows % 2048 == 0 and padded_rows >= n
        pointers, buffer = _upload_filters(store, row_masks + col_masks + [base], padding_set=True)
        for pointer in (pointers[1], pointers[3], pointers[7]):  # padding bits really are set, on both sides and in the base
            assert dense.unpack_bits(store.bitset_download(pointer), padded_rows)[n:].all()
        for base_mask, base_ptr in ((base, pointers[7]), (None, None)):
            table = _cross(store, base_ptr, pointers[:3], pointers[3:7])
            assert table.shape == (3, 4)
            assert np.array_equal(table, cross_filter_counts(base_mask, row_masks, col_masks, n)), base_mask is None
        assert _cross(store, None, [None], [None]).tolist() == [[n]]
        assert _cross(store, pointers[7], [None, pointers[1]], [pointers[3], None]).tolist() == [[int(base.sum())] * 2] * 2
        store.free(buffer)


# ---- b: filters per side around the tile, and at the limit ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid_store(built):
    store = _one_position_store(N_MID)
    yield store
    store.close()


@pytest.mark.parametrize("n_rows,n_cols", [(1, 1), (7, 9), (8, 8), (9, 8), (1, 17), (17, 1), (17, 17), (1024, 3), (3, 1024)])
def test_filter_counts_around_the_tile(mid_store, n_rows, n_cols):
    """Filters per side around the tile of 8 (edge tiles must not read past their arrays) and at the limit of 1 024: random
    densities, an empty, a full and a NULL entry on every side of three or more, with a base and with a NULL base."""
    from silo_amd.binding import CROSS_TILE, MAX_CROSS_FILTERS

    assert CROSS_TILE == 8 and MAX_CROSS_FILTERS == 1024  # what the shapes above stand around
    store = mid_store
    rng = np.random.default_rng(1000 + 31 * n_rows + n_cols)
    row_masks = _random_masks(rng, N_MID, n_rows)
    col_masks = _random_masks(rng, N_MID, n_cols)
    base = rng.random(N_MID) < 0.7
    pointers, buffer = _upload_filters(store, row_masks + col_masks + [base], padding_set=True)
    for base_mask, base_ptr in ((base, pointers[-1]), (None, None)):
        table = _cross(store, base_ptr, pointers[:n_rows], pointers[n_rows:n_rows + n_cols])
        want = cross_filter_counts(base_mask, row_masks, col_masks, N_MID)
        assert want.any()
        assert np.array_equal(table, want), (n_rows, n_cols, base_mask is None)
    store.free(buffer)


# ---- c: the same array on both sides ---------------------------------------------------------------------------------------------
def test_the_same_pointers_on_both_sides(mid_store):
    """11 filters as rows and as columns: the table is symmetric and its diagonal holds the filters' cardinalities under the base."""
    store = mid_store
    rng = np.random.default_rng(92)
    masks = _random_masks(rng, N_MID, 11)
    base = rng.random(N_MID) < 0.6
    pointers, buffer = _upload_filters(store, masks + [base], padding_set=True)
    for base_mask, base_ptr in ((base, pointers[-1]), (None, None)):
        table = _cross(store, base_ptr, pointers[:-1], pointers[:-1])
        assert np.array_equal(table, table.T)
        selected = np.ones(N_MID, bool) if base_mask is None else base_mask
        assert table.diagonal().tolist() == [int((selected if mask is None else selected & mask).sum()) for mask in masks]
        assert np.array_equal(table, cross_filter_counts(base_mask, masks, masks, N_MID))
    store.free(buffer)


# ---- d: cells that several blocks add to ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_store(built):
    store = _one_position_store(N_BIG)
    yield store
    store.close()


@functools.lru_cache(maxsize=None)
def _big_masks():
    rng = np.random.default_rng(93)
    nine = np.zeros(N_BIG, bool)
    nine[rng.choice(N_BIG, size=9, replace=False)] = True
    last = np.zeros(N_BIG, bool)
    last[-3:] = True  # rows of the last, partial chunk only
    return _random_masks(rng, N_BIG, 9) + [nine], _random_masks(rng, N_BIG, 10) + [last], rng.random(N_BIG) < 0.6


def test_cells_summed_over_several_blocks(big_store):
    """140 003 rows, 10 x 11 filters: every cell receives parts from at least three blocks, the last of which covers a partial
    chunk of row words; a base whose words are empty over a stretch (those words read no filter)."""
    from silo_amd.binding import CROSS_CHUNK_WORDS

    store = big_store
    chunks = -(-store.row_words // CROSS_CHUNK_WORDS)
    assert chunks >= 3 and store.row_words % CROSS_CHUNK_WORDS != 0  # blocks per cell; the last chunk is partial
    row_masks, col_masks, base = _big_masks()
    holes = base.copy()
    holes[5_000:80_000] = False
    pointers, buffer = _upload_filters(store, row_masks + col_masks + [base, holes], padding_set=True)
    rows, cols = pointers[:10], pointers[10:21]
    for base_mask, base_ptr in ((None, None), (base, pointers[21]), (holes, pointers[22])):
        table = _cross(store, base_ptr, rows, cols)
        want = cross_filter_counts(base_mask, row_masks, col_masks, N_BIG)
        assert np.array_equal(table, want)
        full_row = [k for k, mask in enumerate(row_masks) if mask is not None and mask.all()][0]
        assert want[full_row, 10] == (3 if base_mask is None else int(base_mask[-3:].sum()))
        # every chunk of rows contributes to the cell of two full entries
        selected = np.ones(N_BIG, bool) if base_mask is None else base_mask
        if base_mask is not holes:
            assert all(selected[c * CROSS_CHUNK_WORDS * 64:(c + 1) * CROSS_CHUNK_WORDS * 64].any() for c in range(chunks))
    store.free(buffer)


# ---- e: index arrays -----------------------------------------------------------------------------------------------------------
def test_index_arrays_permute_scatter_and_fill_sub_blocks(mid_store):
    store = mid_store
    rng = np.random.default_rng(94)
    row_masks = _random_masks(rng, N_MID, 9)
    col_masks = _random_masks(rng, N_MID, 10)
    base = rng.random(N_MID) < 0.7
    pointers, buffer = _upload_filters(store, row_masks + col_masks + [base])
    rows, cols, base_ptr = pointers[:9], pointers[9:19], pointers[19]
    counts = cross_filter_counts(base, row_masks, col_masks, N_MID)
    assert (counts > 0).sum() > 40

    # a permutation on both sides
    row_index, col_index = rng.permutation(9), rng.permutation(10)
    table = _cross(store, base_ptr, rows, cols, row_index=row_index, col_index=col_index)
    want = np.zeros((9, 10), dtype=np.uint32)
    want[np.ix_(row_index, col_index)] = counts
    assert np.array_equal(table, want) and not np.array_equal(table, counts)

    # a scatter into a larger table that starts out non-zero: untouched cells keep their value, touched ones are added to — twice
    shape = (14, 23)
    start = rng.integers(1, 5000, size=shape).astype(np.uint32)
    row_index, col_index = rng.choice(14, size=9, replace=False), rng.choice(23, size=10, replace=False)
    table_dev = store.upload_column(start.reshape(-1))
    want = start.copy()
    for calls in (1, 2):
        assert _cross(store, base_ptr, rows, cols, row_index=row_index, col_index=col_index, out_shape=shape, out_ptr=table_dev) is None
        want[np.ix_(row_index, col_index)] += counts
        assert np.array_equal(store.read(table_dev, np.uint32, start.size).reshape(shape), want)
    untouched = np.ones(shape, bool)
    untouched[np.ix_(row_index, col_index)] = False
    assert untouched.sum() == 14 * 23 - 90 and np.array_equal(want[untouched], start[untouched])
    store.free(table_dev)

    # two calls fill two sub-blocks of one table (rows 0-3 and rows 4-8), an entry left out of the second: its row stays 0
    table_dev = store.upload_column(np.zeros(90, dtype=np.uint32))
    assert _cross(store, base_ptr, rows[:4], cols, row_index=np.arange(4), out_shape=(9, 10), out_ptr=table_dev) is None
    assert _cross(store, base_ptr, rows[4:6] + rows[7:], cols, row_index=[4, 5, 7, 8], out_shape=(9, 10), out_ptr=table_dev) is None
    want = counts.copy()
    want[6] = 0
    assert np.array_equal(store.read(table_dev, np.uint32, 90).reshape(9, 10), want)
    for pointer in (table_dev, buffer):
        store.free(pointer)


# ---- f: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_entry(mid_store):
    """1 025 filters on a side, a NULL table, scratch or filter array, an index at its bound, a repeated index: refused with
    SILO_GPU_ERR_INVALID_ARGUMENT and the table unchanged; no filters on a side: success; the next valid call answers exactly."""
    from silo_amd.binding import MAX_CROSS_FILTERS, SiloGpuError

    invalid_argument = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
    store = mid_store
    rng = np.random.default_rng(95)
    row_masks = _random_masks(rng, N_MID, 3)
    col_masks = _random_masks(rng, N_MID, 4)
    pointers, buffer = _upload_filters(store, row_masks + col_masks)
    rows, cols = pointers[:3], pointers[3:]
    counts = cross_filter_counts(None, row_masks, col_masks, N_MID)
    start = np.full((3, 4), 77, dtype=np.uint32)
    table_dev = store.upload_column(start.reshape(-1))
    refused = [
        dict(row_ptrs=[rows[0]] * (MAX_CROSS_FILTERS + 1), out_shape=(MAX_CROSS_FILTERS + 1, 4), out_ptr=None),
        dict(col_ptrs=[cols[0]] * (MAX_CROSS_FILTERS + 1), out_shape=(3, MAX_CROSS_FILTERS + 1), out_ptr=None),
        dict(out_ptr=ctypes.c_void_p(0)),
        dict(scratch_ptr=None),
        dict(row_ptrs=None),
        dict(col_ptrs=None),
        dict(row_index=[0, 1, 3]),
        dict(col_index=[0, 1, 2, 4]),
        dict(row_index=[0, 1, 1]),
        dict(col_index=[3, 1, 2, 3]),
        dict(out_shape=(2, 4)),  # the identity index of 3 rows in a table of 2
        dict(out_shape=(3, 3)),
    ]
    for options in refused:
        arguments = dict(base_ptr=None, row_ptrs=rows, col_ptrs=cols, out_ptr=table_dev)
        arguments.update(options)
        with pytest.raises(SiloGpuError) as refusal:
            store.filters_cross(**arguments)
        assert refusal.value.code == invalid_argument, options
        assert np.array_equal(store.read(table_dev, np.uint32, 12).reshape(3, 4), start), options
        assert np.array_equal(_cross(store, None, rows, cols), counts), options
    # nothing on a side: success, nothing added
    assert _cross(store, None, [], cols, out_shape=(3, 4), out_ptr=table_dev) is None
    assert _cross(store, None, rows, [], out_shape=(3, 4), out_ptr=table_dev) is None
    assert np.array_equal(store.read(table_dev, np.uint32, 12).reshape(3, 4), start)
    assert _cross(store, None, [], cols).shape == (0, 4) and _cross(store, None, rows, []).shape == (3, 0)
    for pointer in (table_dev, buffer):
        store.free(pointer)


def test_a_store_without_rows_is_refused(built):
    from silo_amd.binding import SiloGpuError
    from tests.test_kernels_gpu import make_store

    with make_store(0, [dict(name="s", alphabet="nuc", reference=np.ones(1, dtype=np.uint8))]) as store:
        table_dev = store.upload_column(np.full(1, 5, dtype=np.uint32))
        with pytest.raises(SiloGpuError) as refusal:
            store.filters_cross(None, [None], [None], out_ptr=table_dev)
        assert refusal.value.code == -1  # SILO_GPU_ERR_INVALID_ARGUMENT
        assert store.read(table_dev, np.uint32, 1).tolist() == [5]
        store.free(table_dev)
