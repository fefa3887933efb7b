"""The grouped filter count (K8, csrc/silo_gpu_grouped.hip) through silo_gpu_filters_grouped, against the numpy reference of
tests/grouped_filters_reference.py (pinned without a GPU by tests/test_grouped_filters_reference.py).

tests/test_queries_over_time_gpu.py reaches K8 through JSON and the engine.  Here the entry point gets the shapes where its
kernels take another path: row counts around a word, the 2 048-row padding and a block of 256 words; words of 64 rows with exactly
4 and exactly 5 ranges (WORD_SEGMENTS); 1, 7, 8, 9, 17 and 2 048 filters (FILTERS_PER_BLOCK); 1, 257 and 1 024 ranges; filters and
a base with their padding bits set; NULL entries and a NULL base; a table that is accumulated into; the refusals of the entry.
Every comparison is an exact integer equality.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402
from tests.grouped_filters_reference import grouped_filter_counts  # noqa: E402
from tests.test_grouped_kernels_gpu import (  # noqa: E402
    N_RANGES, N_ROWS, _date_columns, _distinct_ranges_per_word, _ranges, _short_ranges)
from tests.test_kernels_gpu import NUC_CHARS, make_store  # noqa: E402

NO_GROUP = dense.NO_GROUP
UNBOUNDED = 0xFFFFFFFF
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _one_position_store(n):
    """A finalized store of n rows (one nucleotide position: K8 reads none of it, only row_words and sequence_count)."""
    store = make_store(n, [dict(name="s", alphabet="nuc", reference=np.ones(1, dtype=np.uint8))])
    try:
        store.append_sequences(0, 0, NUC_CHARS[np.ones((n, 1), dtype=np.uint8)])
        store.finalize()
    except Exception:
        store.close()
        raise
    return store


def _padded_words(store, mask, padding_set):
    """The mask as row_words words; padding_set: every bit at or past len(mask) is set."""
    words = np.zeros(store.row_words, dtype=np.uint64)
    packed = dense.pack_bits(mask)
    words[:len(packed)] = packed
    if padding_set:
        n = len(mask)
        if n % 64:
            words[n // 64] |= ALL_ONES << np.uint64(n % 64)
        words[-(-n // 64):] = ALL_ONES
    return words


def _upload_filters(store, masks, padding_set=False):
    """One device buffer for all masks (None stays None): the device pointers in order, and the buffer to free."""
    present = [mask for mask in masks if mask is not None]
    if not present:
        return [None] * len(masks), None
    words = np.stack([_padded_words(store, mask, padding_set) for mask in present])
    buffer = store.malloc(words.nbytes)
    assert store.lib.silo_gpu_memcpy_h2d(buffer, words.ctypes.data_as(ctypes.c_void_p), words.nbytes, None) == 0
    store.synchronize()
    pointers, k = [], 0
    for mask in masks:
        if mask is None:
            pointers.append(None)
        else:
            pointers.append(ctypes.c_void_p(buffer.value + k * store.row_words * 8))
            k += 1
    return pointers, buffer


def _random_masks(rng, n, count):
    """`count` masks of random densities; among them (from three on) an empty one, a full one and a None entry."""
    masks = [rng.random(n) < density for density in rng.random(count)]
    if count >= 3:
        picks = rng.choice(count, size=3, replace=False)
        masks[picks[0]], masks[picks[1]], masks[picks[2]] = np.zeros(n, bool), np.ones(n, bool), None
    return masks


# ---- a: row counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 16_385])
def test_row_counts_and_padding_bits(built, n):
    """3 filters x 5 ranges at row counts around a word, the 2 048-row padding and a block of 256 words; the filters and the base
    have every padding bit set: rows past sequence_count never count, and have no range in the scratch."""
    rng = np.random.default_rng(500 + n)
    ranges = [(100, 150), (151, 300), (0, 50), (400, UNBOUNDED), (60, 60)]
    dates = rng.integers(0, 450, size=n).astype(np.uint32)
    dates[rng.random(n) < 0.1] = 0
    masks = [rng.random(n) < 0.5, np.ones(n, bool), rng.random(n) < 0.1]
    base = rng.random(n) < 0.8
    with _one_position_store(n) as store:
        padded_rows = store.row_words * 64
        assert padded_rows % 2048 == 0 and padded_rows >= n
        pointers, buffer = _upload_filters(store, masks + [base], padding_set=True)
        assert dense.unpack_bits(store.bitset_download(pointers[1]), padded_rows).all()  # padding bits really are set
        dates_dev = store.upload_column(dates)
        for base_mask, base_ptr in ((base, pointers[3]), (None, None)):
            table, groups = store.filters_grouped(base_ptr, dates_dev, ranges, pointers[:3], return_groups=True)
            assert table.shape == (3, 5) and groups.shape == (padded_rows,)
            assert np.array_equal(table, grouped_filter_counts(base_mask, masks, dates, ranges))
            assert np.array_equal(groups[:n], dense.row_groups(np.ones(n, bool) if base_mask is None else base_mask, dates, ranges))
            assert (groups[n:] == NO_GROUP).all()
        store.free(dates_dev)
        store.free(buffer)


# ---- b: word decoding ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_store(built):
    store = _one_position_store(N_ROWS)
    yield store
    store.close()


@functools.lru_cache(maxsize=None)
def _big_masks():
    rng = np.random.default_rng(51)
    masks = _random_masks(rng, N_ROWS, 9)
    nine = np.zeros(N_ROWS, bool)
    nine[rng.choice(N_ROWS, size=9, replace=False)] = True
    masks[[k for k, mask in enumerate(masks) if mask is not None and mask.any() and not mask.all()][0]] = nine
    return masks, rng.random(N_ROWS) < 0.6


def test_word_decoding_on_both_sides_of_the_segments(big_store):
    """70 001 rows, 40 ranges, 9 filters (two blocks of 8), with and without a base, over three date columns: sorted in blocks
    (words of one or two ranges: the segment path), uniformly random (row by row) and one built so that word w holds exactly
    w % 7 + 1 ranges — words of exactly 4 (the last on the segment path) and exactly 5 (the first row by row) exist."""
    store = big_store
    ranges = _ranges()
    masks, base = _big_masks()
    pointers, buffer = _upload_filters(store, masks + [base])
    everyone = np.ones(N_ROWS, bool)
    for column_index, dates in enumerate(_date_columns()):
        dates_dev = store.upload_column(dates)
        for base_mask, base_ptr in ((None, None), (base, pointers[-1])):
            want_groups = dense.row_groups(everyone if base_mask is None else base_mask, dates, ranges)
            distinct, _ = _distinct_ranges_per_word(want_groups)
            if column_index == 0:
                assert (distinct <= 4).mean() > 0.9 and (distinct >= 2).any()
            if column_index == 1:
                assert (distinct > 4).mean() > 0.9
            if column_index == 2:
                assert all((distinct == exactly).any() for exactly in (1, 2, 3, 4, 5, 7))
            table, groups = store.filters_grouped(base_ptr, dates_dev, ranges, pointers[:-1], return_groups=True)
            assert table.shape == (9, N_RANGES)
            assert np.array_equal(groups[:N_ROWS], want_groups) and (groups[N_ROWS:] == NO_GROUP).all()
            want = grouped_filter_counts(base_mask, masks, dates, ranges)
            assert np.array_equal(table, want), (column_index, base_mask is None)
            assert want.any(axis=1).sum() == 8  # every filter but the empty one counts somewhere
        store.free(dates_dev)
    store.free(buffer)


# ---- c: filter counts, range counts ------------------------------------------------------------------------------------------
N_MID = 20_001  # two blocks of 256 words


@pytest.fixture(scope="module")
def mid_store(built):
    store = _one_position_store(N_MID)
    yield store
    store.close()


@functools.lru_cache(maxsize=None)
def _mid_dates():
    rng = np.random.default_rng(52)
    last_day = 2000 + 5 * 1024 + 20  # past the last of 1 024 ranges of _short_ranges
    sorted_days = np.sort(rng.integers(1990, last_day, size=N_MID))
    sorted_days[rng.choice(N_MID, size=300, replace=False)] = 0
    shuffled = rng.integers(1990, last_day, size=N_MID)
    shuffled[rng.choice(N_MID, size=300, replace=False)] = 0
    return sorted_days.astype(np.uint32), shuffled.astype(np.uint32)


@pytest.mark.parametrize("n_filters", [1, 7, 8, 9, 17, 2048])
def test_filter_counts_around_the_block_batch(mid_store, n_filters):
    """1, 7, 8, 9, 17 and 2 048 filters of random densities, an empty one, a full one and a NULL entry among them, with a base
    and with a NULL base, over 5 ranges."""
    store = mid_store
    rng = np.random.default_rng(600 + n_filters)
    ranges = [(2100, 2400), (2401, 2401), (0, 2050), (3500, UNBOUNDED), (2500, 3000)]
    masks = _random_masks(rng, N_MID, n_filters)
    if n_filters == 1:
        masks = [rng.random(N_MID) < 0.3]
    base = rng.random(N_MID) < 0.7
    pointers, buffer = _upload_filters(store, masks + [base])
    for dates in _mid_dates():
        dates_dev = store.upload_column(dates)
        for base_mask, base_ptr in ((base, pointers[-1]), (None, None)):
            table = store.filters_grouped(base_ptr, dates_dev, ranges, pointers[:-1])
            want = grouped_filter_counts(base_mask, masks, dates, ranges)
            assert want.any()
            assert np.array_equal(table, want), (n_filters, base_mask is None)
        store.free(dates_dev)
    # only NULL entries: every filter is all rows
    dates_dev = store.upload_column(_mid_dates()[0])
    table = store.filters_grouped(pointers[-1], dates_dev, ranges, [None] * min(n_filters, 9))
    assert np.array_equal(table, grouped_filter_counts(base, [None] * min(n_filters, 9), _mid_dates()[0], ranges))
    store.free(dates_dev)
    store.free(buffer)


def _day_ranges(rng, count):
    """`count` ranges of 1-3 days from day 2000 on, touching or a day or two apart, in shuffled request order; from three on the
    earliest is unbounded below and the latest unbounded above."""
    ranges = _short_ranges(rng, count)
    if count >= 3:
        first = min(range(count), key=lambda k: ranges[k][0])
        last = max(range(count), key=lambda k: ranges[k][0])
        ranges[first] = (0, ranges[first][1])
        ranges[last] = (ranges[last][0], UNBOUNDED)
    return ranges


@pytest.mark.parametrize("n_ranges,n_filters", [(1, 9), (257, 9), (1024, 9), (1024, 2048)])
def test_range_counts(mid_store, n_ranges, n_filters):
    """1, 257 and 1 024 ranges in shuffled request order, touching and unbounded ones among them (the LDS histogram and the bounds
    are strided over by 256 threads), once with sorted dates (segments) and once with random ones (row by row); one run with 1 024
    ranges x 2 048 filters."""
    store = mid_store
    rng = np.random.default_rng(700 + n_ranges + n_filters)
    ranges = _day_ranges(rng, n_ranges) if n_ranges > 1 else [(2100, 2600)]
    masks = _random_masks(rng, N_MID, n_filters)
    base = rng.random(N_MID) < 0.7
    pointers, buffer = _upload_filters(store, masks + [base])
    columns = _mid_dates() if n_filters <= 9 else _mid_dates()[1:]
    for column_index, dates in enumerate(columns):
        base_mask, base_ptr = ((base, pointers[-1]), (None, None))[column_index % 2]
        dates_dev = store.upload_column(dates)
        table, groups = store.filters_grouped(base_ptr, dates_dev, ranges, pointers[:-1], return_groups=True)
        assert table.shape == (n_filters, n_ranges)
        assert np.array_equal(groups[:N_MID], dense.row_groups(np.ones(N_MID, bool) if base_mask is None else base_mask, dates, ranges))
        want = grouped_filter_counts(base_mask, masks, dates, ranges)
        assert (want.max(axis=0) > 0).mean() > 0.9  # nearly every range is reached
        assert np.array_equal(table, want)
        store.free(dates_dev)
    store.free(buffer)


# ---- d: accumulation ---------------------------------------------------------------------------------------------------------
def test_the_table_is_accumulated_into(mid_store):
    """A table that starts out as a constant: constant + counts after one call, constant + 2 x counts after a second; a call
    without ranges or without filters succeeds and leaves it as it is."""
    store = mid_store
    rng = np.random.default_rng(53)
    ranges = _day_ranges(rng, 12)
    masks = _random_masks(rng, N_MID, 11)
    pointers, buffer = _upload_filters(store, masks)
    dates = _mid_dates()[0]
    dates_dev = store.upload_column(dates)
    counts = grouped_filter_counts(None, masks, dates, ranges)
    assert counts.any()
    start = np.full(counts.shape, 1000, dtype=np.uint32)
    table_dev = store.upload_column(start.reshape(-1))
    for calls in (1, 2):
        assert store.filters_grouped(None, dates_dev, ranges, pointers, out_ptr=table_dev) is None
        assert np.array_equal(store.read(table_dev, np.uint32, start.size).reshape(start.shape), start + calls * counts)
    assert store.filters_grouped(None, dates_dev, [], pointers, out_ptr=table_dev) is None
    assert store.filters_grouped(None, dates_dev, ranges, [], out_ptr=table_dev) is None
    assert np.array_equal(store.read(table_dev, np.uint32, start.size).reshape(start.shape), start + 2 * counts)
    assert store.filters_grouped(None, dates_dev, [], pointers).shape == (11, 0)
    assert store.filters_grouped(None, dates_dev, ranges, []).shape == (0, 12)
    for pointer in (table_dev, dates_dev, buffer):
        store.free(pointer)


# ---- e: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_entry(mid_store):
    """1 025 ranges, 2 049 filters, overlapping ranges, ranges that share a day, from > to, a NULL scratch, table, date column or
    filter array are refused with an error status; the next valid call on the store answers exactly."""
    from silo_amd.binding import MAX_DATE_RANGES, MAX_GROUPED_FILTERS, SiloGpuError

    store = mid_store
    rng = np.random.default_rng(54)
    masks = _random_masks(rng, N_MID, 9)
    pointers, buffer = _upload_filters(store, masks)
    dates = _mid_dates()[1]
    dates_dev = store.upload_column(dates)
    good = [(2100, 2200), (2201, 2300), (0, 2000)]
    want = grouped_filter_counts(None, masks, dates, good)
    refused = [
        dict(ranges=[(3000 + k, 3000 + k) for k in range(MAX_DATE_RANGES + 1)]),
        dict(filter_ptrs=[pointers[0]] * (MAX_GROUPED_FILTERS + 1)),
        dict(ranges=[(2100, 2200), (2150, 2300)]),
        dict(ranges=[(2250, 2300), (2100, 2260)]),   # overlapping, given in descending order
        dict(ranges=[(2100, 2200), (2200, 2300)]),   # to == the next from: both ends are inclusive
        dict(ranges=[(2200, 2100)]),
        dict(scratch_ptr=None),
        dict(out_ptr=ctypes.c_void_p(0), return_groups=True),  # (a null table; the groups so that nothing reads the table back)
        dict(dates_ptr=None),
        dict(filter_ptrs=None),
    ]
    for options in refused:
        arguments = dict(base_ptr=None, dates_ptr=dates_dev, ranges=good, filter_ptrs=pointers)
        arguments.update(options)
        with pytest.raises(SiloGpuError) as refusal:
            store.filters_grouped(**arguments)
        assert refusal.value.code < 0, options
        assert np.array_equal(store.filters_grouped(None, dates_dev, good, pointers), want), options
    for pointer in (dates_dev, buffer):
        store.free(pointer)
