"""silo_gpu_nearest_rows (K11, csrc/silo_gpu_nearest.hip) called directly on tables made in numpy — it takes no store — against
the sort-everything reference of tests/nearest_rows_reference.py (pinned without a GPU by tests/test_nearest_rows_reference.py).
The list is filled with 0xA5 before every call: entries past the count must still hold it.  Exact integer equality throughout."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import nearest_rows_reference as ref  # noqa: E402

FILL = 0xA5
UNTOUCHED = 0xA5A5A5A5
NO_ROW = ref.NO_ROW


def _pack(mask, padded_rows=None, pad_with=False):
    """A row bitset of whole words; the bits at or past len(mask) are set where pad_with."""
    rows = -(-len(mask) // 64) * 64 if padded_rows is None else padded_rows
    bits = np.full(rows, pad_with, dtype=bool)
    bits[:len(mask)] = mask
    return np.packbits(bits, bitorder="little").view("<u8")


def _call(table, mask, k, max_distance=NO_ROW, exclude=NO_ROW, filter_words="from mask"):
    from silo_amd import binding

    words = (None if mask is None else _pack(mask)) if isinstance(filter_words, str) else filter_words
    return binding.nearest_rows(table, words, len(table), k, exclude_row=exclude, max_distance=max_distance, fill=FILL)


def _check(table, mask, k, max_distance=NO_ROW, exclude=NO_ROW, what=None, **options):
    count, listed = _call(table, mask, k, max_distance, exclude, **options)
    want = ref.nearest_list(table, ref.nearest(table, mask, k, max_distance, exclude))
    assert count == len(want), (what, count, len(want))
    assert np.array_equal(listed[:count], want), what
    assert (listed[count:] == UNTOUCHED).all(), what  # entries past the count are not touched
    return count, listed


@functools.lru_cache(maxsize=None)
def _table(n):
    """Distances as a store of a few hundred positions gives them: many rows per value, a few rows close by."""
    rng = np.random.default_rng(50 + n)
    table = np.column_stack([rng.integers(0, 300, size=n), rng.integers(250, 400, size=n)]).astype(np.uint32)
    table.setflags(write=False)
    return table


@pytest.mark.parametrize("k", [1, 10, 1024])
@pytest.mark.parametrize("n", [1, 64, 65, 70_001])
def test_matches_sorting_everything(built, n, k):
    table = _table(n)
    rng = np.random.default_rng(n + k)
    _check(table, None, k, what="no filter")
    _check(table, rng.random(n) < 0.5, k, what="random filter")
    _check(table, np.zeros(n, bool), k, what="empty filter")
    few = np.zeros(n, bool)
    few[rng.choice(n, size=min(n, 7), replace=False)] = True  # fewer rows than k (for k >= 10)
    _check(table, few, k, what="few rows")
    # padding bits set past sequence_count never select a row
    everyone = np.ones(n, bool)
    _check(table, everyone, k, what="padding bits", filter_words=_pack(everyone, -(-n // 2048) * 2048, pad_with=True))
    kth = int(np.sort(table[:, 0])[min(k, n) - 1])
    for bound in (kth, max(kth, 1) - 1, 0):  # at and below the k-th distance
        _check(table, None, k, max_distance=bound, what=("max distance", bound))
    inside = int(np.argmin(table[:, 0]))  # the nearest row of all
    _check(table, None, k, exclude=inside, what="excluded row")
    outside = np.ones(n, bool)
    outside[inside] = False
    _check(table, outside, k, exclude=inside, what="excluded row outside the filter")
    _check(table, None, k, exclude=n + 5, what="excluded row past the table")


def test_all_rows_at_distance_zero(built):
    n = 70_001
    table = np.zeros((n, 2), dtype=np.uint32)
    table[:, 1] = np.arange(n) % 97
    for k in (1, 10, 1024):
        count, listed = _check(table, None, k, what=k)
        assert count == k and np.array_equal(listed[:k, 0], np.arange(k))


def test_ties_at_the_kth_distance_go_to_the_lowest_rows(built):
    """3 rows below, 5 000 rows tied at the k-th distance, the others above: the chosen ones are the tied rows with the lowest ids."""
    n, k = 70_001, 10
    rng = np.random.default_rng(8)
    table = np.column_stack([rng.integers(50, 90, size=n), rng.integers(0, 1000, size=n)]).astype(np.uint32)
    tied = np.sort(rng.choice(n, size=5000, replace=False))
    table[tied, 0] = 40
    below = np.setdiff1d(rng.choice(n, size=20, replace=False), tied)[:3]
    table[below, 0] = [7, 3, 7]
    count, listed = _check(table, None, k, what="ties")
    assert count == k and sorted(listed[:3, 0].tolist()) == sorted(below.tolist())
    assert np.array_equal(listed[3:k, 0], tied[:k - 3])
    mask = np.ones(n, bool)
    mask[tied[:4000]] = False
    _, listed = _check(table, mask, 1024, what="ties under a filter")
    assert np.array_equal(listed[3:1003, 0], tied[4000:])


def test_distances_above_16_bits(built):
    n = 5000
    rng = np.random.default_rng(4)
    table = np.column_stack([rng.integers(60_000, 4_000_000_000, size=n, dtype=np.int64), rng.integers(0, 1 << 32, size=n, dtype=np.int64)]).astype(np.uint32)
    table[17, 0] = 0xFFFFFFFF
    assert (table[:, 0] > 65_535).sum() > n // 2
    for k in (1, 10, 1024):
        _check(table, None, k, what=k)
        _check(table, rng.random(n) < 0.3, k, max_distance=2_000_000_000, what=(k, "bounded"))
    count, listed = _check(table, np.arange(n) == 17, 10, what="the largest distance")
    assert count == 1 and listed[0].tolist() == [17, 0xFFFFFFFF, int(table[17, 1])]


def test_two_runs_give_identical_output(built):
    table = _table(70_001)
    mask = np.random.default_rng(1).random(len(table)) < 0.7
    first = _call(table, mask, 1024)
    second = _call(table, mask, 1024)
    assert first[0] == second[0] == 1024 and np.array_equal(first[1], second[1])


def test_refusals_write_nothing(built):
    from silo_amd import binding

    table = np.ascontiguousarray(_table(65))
    table_dev = binding.device_malloc(table.nbytes)
    binding._check(binding.load_library().silo_gpu_memcpy_h2d(table_dev, binding._ptr(table), table.nbytes, None))
    out = binding.device_malloc(1024 * 12, FILL)
    count = binding.device_malloc(4, FILL)
    scratch = binding.device_malloc(binding.NEAREST_ROWS_SCRATCH_BYTES, FILL)
    try:
        good = dict(table_ptr=table_dev, filter_ptr=None, sequence_count=65, exclude_row=NO_ROW, max_distance=NO_ROW, k=10, out_ptr=out,
                    count_ptr=count, scratch_ptr=scratch)
        for change in (dict(table_ptr=None), dict(out_ptr=None), dict(count_ptr=None), dict(scratch_ptr=None), dict(k=0),
                       dict(k=binding.MAX_NEAREST_ROWS + 1), dict(sequence_count=0)):
            with pytest.raises(binding.SiloGpuError):
                binding.nearest_rows_call(**{**good, **change})
        assert (binding.device_read(out, np.uint8, 1024 * 12) == FILL).all()
        assert (binding.device_read(count, np.uint8, 4) == FILL).all()
        assert (binding.device_read(scratch, np.uint8, binding.NEAREST_ROWS_SCRATCH_BYTES) == FILL).all()
        binding.nearest_rows_call(**good)  # the same buffers serve a good call
        assert int(binding.device_read(count, np.uint32, 1)[0]) == 10
        want = ref.nearest_list(table, ref.nearest(table, None, 10))
        assert np.array_equal(binding.device_read(out, np.uint32, 30).reshape(10, 3), want)
    finally:
        for ptr in (table_dev, out, count, scratch):
            binding.device_free(ptr)
