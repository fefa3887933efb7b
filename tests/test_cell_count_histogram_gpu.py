"""silo_gpu_cell_count_histogram (K22, behind the action CellCountDistribution) alone, on tables and filters made in numpy: it adds, per
selected row r < sequence_count, one to bin min(value(r) / bin_width, n_bins - 1).  The expected bins are np.bincount
(tests/cell_counts_reference.py); every comparison is an exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cell_counts_reference as ref  # noqa: E402
from tests.test_bitset_from_cell_counts_gpu import SIZES, make_table, row_words_of, words_of  # noqa: E402

GUARD_WORDS = 4
GUARD = np.full(GUARD_WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
MASK = 5            # substitutions + missing: values in [0, 339)
LARGEST = 39 + 299  # the largest value MASK can give on make_table
BIN_WIDTHS = [1, 7, LARGEST + 1]
BIN_COUNTS = [1, 2, 256, 4096]


def filters_of(n, row_words):
    """(name, uint64 [row_words] or None, bool [row_words * 64] of the rows that count)."""
    rows = row_words * 64
    real = np.arange(rows) < n
    rng = np.random.default_rng(n)
    half = rng.random(rows) < 0.5
    sparse = np.arange(rows) % 500 == 3 % max(n, 1)
    one = np.arange(rows) == n - 1
    out = [("null", None, real), ("all", np.ones(rows, dtype=bool), real), ("half", half, half & real), ("1-in-500", sparse, sparse & real),
           ("one-row", one, one), ("none", np.zeros(rows, dtype=bool), np.zeros(rows, dtype=bool)), ("padding-bits", ~real, np.zeros(rows, dtype=bool))]
    return [(name, None if bits is None else words_of(bits), counting) for name, bits, counting in out]


def _run(parts, mask, bin_width, n_bins, initial=None):
    from silo_amd import binding

    out = binding.cell_count_histogram(parts, mask, bin_width, n_bins, initial=initial, guard_words=GUARD_WORDS)
    assert np.array_equal(out[n_bins:], GUARD), "words past n_bins were touched"
    return out[:n_bins]


def _part(table, n, row_words, filter_words):
    return dict(table=table, row_words=row_words, sequence_count=n, filter=filter_words)


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_filters(built, n, rounded):
    row_words = row_words_of(n, rounded)
    table = make_table(n, row_words)
    for name, filter_words, counting in filters_of(n, row_words):
        want = ref.bins(table, counting, MASK, 7, 256)
        assert int(want.sum()) == int(counting.sum())
        assert np.array_equal(_run([_part(table, n, row_words, filter_words)], MASK, 7, 256), want), (n, row_words, name)


@pytest.mark.parametrize("n_bins", BIN_COUNTS)
@pytest.mark.parametrize("bin_width", BIN_WIDTHS)
def test_bin_widths_and_bin_counts(built, bin_width, n_bins):
    n = 70_001
    row_words = row_words_of(n, True)
    table = make_table(n, row_words)
    half = filters_of(n, row_words)[2]
    for mask in (MASK, 8, 15):
        want = ref.bins(table, half[2], mask, bin_width, n_bins)
        assert np.array_equal(_run([_part(table, n, row_words, half[1])], mask, bin_width, n_bins), want), (mask, bin_width, n_bins)
    want = ref.bins(table, half[2], MASK, bin_width, n_bins)
    if bin_width * n_bins <= LARGEST:  # values beyond the last bin land in it
        assert want[-1] > int((ref.values(table, MASK)[half[2]] // np.uint64(bin_width) == n_bins - 1).sum())
    if bin_width == LARGEST + 1 or n_bins == 1:  # all rows in one bin: a wave adds once
        assert want[0] == int(half[2].sum()) and not want[1:].any()


def test_all_rows_in_different_bins_and_in_one(built):
    n = 4096
    row_words = row_words_of(n, False)
    table = np.zeros((row_words * 64, 4), dtype=np.uint32)
    table[:, 2] = np.random.default_rng(4).permutation(n)  # a wave's 64 rows in 64 bins
    got = _run([_part(table, n, row_words, None)], 4, 1, 4096)
    assert np.array_equal(got, np.ones(4096, dtype=np.uint64))
    table[:, 2] = 17
    got = _run([_part(table, n, row_words, None)], 4, 1, 4096)
    assert got[17] == n and int(got.sum()) == n
    table[:, 2] = np.arange(n) // 2048  # two bins, each of 32 whole waves
    assert _run([_part(table, n, row_words, None)], 4, 1, 2).tolist() == [2048, 2048]
    table[:, 2] = np.arange(n) % 2      # two bins in every wave
    assert _run([_part(table, n, row_words, None)], 4, 1, 2).tolist() == [2048, 2048]


def test_values_near_2_to_the_32(built):
    n = 130
    row_words = row_words_of(n, False)
    table = np.zeros((row_words * 64, 4), dtype=np.uint32)
    table[:n] = 0xFFFFFFFF  # 4 * (2^32 - 1) under mask 15
    table[64:n, 1:] = 0     # 2^32 - 1
    for bin_width, n_bins in ((0xFFFFFFFF, 8), (1, 4096), (0x80000000, 16)):
        want = ref.bins(table, np.arange(row_words * 64) < n, 15, bin_width, n_bins)
        assert np.array_equal(_run([_part(table, n, row_words, None)], 15, bin_width, n_bins), want), (bin_width, n_bins)
    assert ref.bins(table, np.arange(row_words * 64) < n, 15, 0xFFFFFFFF, 8).tolist() == [0, 66, 0, 0, 64, 0, 0, 0]


def test_parts_accumulate_and_bins_are_added_to(built):
    parts, want = [], np.zeros(256, dtype=np.uint64)
    for n, which in ((2049, 2), (65, 0), (70_001, 3)):
        row_words = row_words_of(n, True)
        table = make_table(n, row_words, seed=9)
        _, filter_words, counting = filters_of(n, row_words)[which]
        parts.append(_part(table, n, row_words, filter_words))
        want += ref.bins(table, counting, MASK, 3, 256)
    assert (want > 0).sum() > 50
    assert np.array_equal(_run(parts, MASK, 3, 256), want)
    initial = np.arange(256, dtype=np.uint64) * np.uint64(1 << 33) + np.uint64(5)  # beyond 32 bits: the adds are 64-bit
    assert np.array_equal(_run(parts, MASK, 3, 256, initial=initial), want + initial)


def test_refusals_write_nothing(built):
    from silo_amd import binding

    n, row_words, n_bins = 65, 2, 16
    table = make_table(n, row_words)
    table_dev = binding._upload(table)
    filter_dev = binding._upload(words_of(np.ones(row_words * 64, dtype=bool)))
    bins = binding.device_malloc((n_bins + GUARD_WORDS) * 8, 0xA5)
    try:
        good = dict(table_ptr=table_dev, row_words=row_words, sequence_count=n, filter_ptr=filter_dev, kinds_mask=MASK, bin_width=30, n_bins=n_bins,
                    bins_ptr=bins)
        for change in (dict(table_ptr=None), dict(bins_ptr=None), dict(row_words=0), dict(sequence_count=0), dict(sequence_count=row_words * 64 + 1),
                       dict(kinds_mask=0), dict(kinds_mask=16), dict(bin_width=0), dict(n_bins=0), dict(n_bins=binding.MAX_CELL_COUNT_BINS + 1)):
            with pytest.raises(binding.SiloGpuError):
                binding.cell_count_histogram_call(**{**good, **change})
        assert (binding.device_read(bins, np.uint8, (n_bins + GUARD_WORDS) * 8) == 0xA5).all()
        binding._check(binding.load_library().silo_gpu_memset_async(bins, 0, n_bins * 8, None))
        binding.cell_count_histogram_call(**good)  # the same buffers serve a good call
        got = binding.device_read(bins, np.uint64, n_bins + GUARD_WORDS)
        assert np.array_equal(got[:n_bins], ref.bins(table, np.arange(row_words * 64) < n, MASK, 30, n_bins)) and np.array_equal(got[n_bins:], GUARD)
    finally:
        for ptr in (table_dev, filter_dev, bins):
            binding.device_free(ptr)
