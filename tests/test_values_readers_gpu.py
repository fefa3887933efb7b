"""silo_gpu_bitset_from_values and silo_gpu_count_values (K23, the two readers of value columns) alone, on columns made in numpy:
bit r of the bitset is r < sequence_count and at_least <= values[r] <= at_most; the count of a column is the number of such rows
under a filter, ADDED to what the array held.  The expected words and counts come from tests/region_counts_reference.py; every
comparison is an exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import region_counts_reference as ref  # noqa: E402

FILL = 0xA5
GUARD_WORDS = 4
GUARD = np.full(GUARD_WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
NO_BOUND = 0xFFFFFFFF
SIZES = [1, 63, 64, 65, 70_001]
PADDING = 0xFFFFFFFF  # the cells of a padding row: inside every interval that ends at 2^32 - 1


def row_words_of(n, rounded):
    words = (n + 63) // 64
    return (words + 31) // 32 * 32 if rounded else words


def make_columns(n, row_words, n_columns=1, seed=0):
    """uint32 [n_columns][row_words * 64]: column c holds values in [0, 30 + 7 c) for the n rows (a third of them 0, row 0 holds
    2^32 - 1 where there is more than one row), PADDING behind them."""
    rng = np.random.default_rng(4000 + seed + n)
    columns = np.full((n_columns, row_words * 64), PADDING, dtype=np.uint32)
    for c in range(n_columns):
        columns[c, :n] = rng.integers(0, 30 + 7 * c, size=n) * (rng.random(n) > 0.33)
    if n > 1:
        columns[:, 0] = NO_BOUND
    return columns


def bounds_of(column, n):
    """(at_least, at_most) pairs at, one below and one above values present, with 0, 2^32 - 1 and an empty interval."""
    present = np.unique(column[:n])
    middle = int(present[len(present) // 2])
    return [(0, NO_BOUND), (0, middle), (middle, NO_BOUND), (middle, middle), (max(middle - 1, 0), middle + 1), (middle + 1, NO_BOUND),
            (0, max(middle - 1, 0)), (0, 0), (NO_BOUND, NO_BOUND), (middle + 1, middle), (1, NO_BOUND - 1)]


def filters_of(n, row_words, seed=0):
    """name -> uint64 [row_words] or None: every row, no row, only padding bits, random bits (padding bits set too)."""
    rng = np.random.default_rng(4100 + seed + n)
    padding_only = ~ref.bitset_words(np.ones(n, dtype=bool), row_words)
    random_bits = rng.integers(0, 1 << 63, size=row_words, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=row_words, dtype=np.uint64)
    return {"null": None, "empty": np.zeros(row_words, dtype=np.uint64), "all-padding": padding_only, "random": random_bits | padding_only}


def rows_of(filter_words, total_rows):
    if filter_words is None:
        return np.ones(total_rows, dtype=bool)
    return np.unpackbits(filter_words.view(np.uint8), bitorder="little").astype(bool)[:total_rows]


def _bitset(column, n, row_words, at_least=0, at_most=NO_BOUND):
    from silo_amd import binding

    out = binding.bitset_from_values(column, row_words, n, at_least, at_most, fill=FILL, guard_words=GUARD_WORDS)
    assert np.array_equal(out[row_words:], GUARD), "words past row_words were touched"
    return out[:row_words]


def _counts(parts, bounds, initial=None):
    from silo_amd import binding

    out = binding.count_values(parts, bounds, initial=initial, guard_words=GUARD_WORDS, fill=FILL)
    assert np.array_equal(out[len(bounds):], GUARD), "words past the counts were touched"
    return out[:len(bounds)]


def want_counts(parts, bounds, initial=None):
    total = np.zeros(len(bounds), dtype=np.uint64) if initial is None else np.array(initial, dtype=np.uint64)
    for part in parts:
        columns = np.asarray(part["values"]).reshape(len(bounds), -1)
        rows = rows_of(part["filter"], columns.shape[1]) & (np.arange(columns.shape[1]) < part["sequence_count"])
        total = total + ref.counts(columns, rows, bounds)
    return total


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
@pytest.mark.parametrize("n", SIZES)
def test_bitset_every_word_is_written_and_padding_rows_are_clear(built, n, rounded):
    row_words = row_words_of(n, rounded)
    column = make_columns(n, row_words)[0]
    for at_least, at_most in bounds_of(column, n):
        want = ref.bitset_words(ref.selected(column, n, at_least, at_most), row_words)
        assert np.array_equal(_bitset(column, n, row_words, at_least, at_most), want), (n, row_words, at_least, at_most)
    everything = _bitset(column, n, row_words)  # exactly the n real rows, although every padding cell passes
    assert np.array_equal(everything, ref.bitset_words(np.ones(n, dtype=bool), row_words))


def test_bitset_bounds_cut_on_the_large_column():
    n = 70_001
    column = make_columns(n, row_words_of(n, True))[0]
    counts = [int(ref.selected(column, n, low, high).sum()) for low, high in bounds_of(column, n)]
    assert counts[0] == n and 0 < counts[1] < n and 0 < counts[2] < n and 0 < counts[3] < counts[1] and 0 < counts[7] < n
    assert counts[8] == 1 and counts[9] == 0 and 0 < counts[10] < n  # row 0 holds 2^32 - 1


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
@pytest.mark.parametrize("n", SIZES)
def test_counts_under_every_filter_and_bound(built, n, rounded):
    row_words = row_words_of(n, rounded)
    columns = make_columns(n, row_words, 2)
    pairs = list(zip(bounds_of(columns[0], n), reversed(bounds_of(columns[1], n))))  # two columns with different bounds each
    for name, filter_words in filters_of(n, row_words).items():
        for bounds in pairs:
            part = dict(values=columns, row_words=row_words, sequence_count=n, filter=filter_words)
            assert np.array_equal(_counts([part], bounds), want_counts([part], bounds)), (n, row_words, name, bounds)
    one = dict(values=columns[:1], row_words=row_words, sequence_count=n, filter=None)
    assert _counts([one], [(0, NO_BOUND)]).tolist() == [n]  # padding rows never count, although their cells pass


def test_256_columns_with_bounds_of_their_own(built):
    n = 2049
    row_words = row_words_of(n, False)
    columns = make_columns(n, row_words, ref.MAX_REGIONS)
    bounds = [(c % 5, 3 + c % 29) for c in range(ref.MAX_REGIONS)]
    bounds[7], bounds[8], bounds[9] = (0, NO_BOUND), (NO_BOUND, NO_BOUND), (5, 4)
    for name, filter_words in filters_of(n, row_words).items():
        part = dict(values=columns, row_words=row_words, sequence_count=n, filter=filter_words)
        want = want_counts([part], bounds)
        assert np.array_equal(_counts([part], bounds), want), name
        if name == "null":
            assert want[7] == n and want[8] == 1 and want[9] == 0 and len(np.unique(want)) > 20
        if name in ("empty", "all-padding"):
            assert not want.any()


def test_two_parts_accumulate_into_counts_that_were_not_cleared(built):
    parts = []
    for n, rounded, seed in ((70_001, True, 1), (65, False, 2)):
        row_words = row_words_of(n, rounded)
        parts.append(dict(values=make_columns(n, row_words, 2, seed), row_words=row_words, sequence_count=n, filter=filters_of(n, row_words, seed)["random"]))
    bounds = [(1, 12), (0, 0)]
    initial = np.array([5, (1 << 40) + 3], dtype=np.uint64)
    want = want_counts(parts, bounds, initial)
    assert np.array_equal(_counts(parts, bounds, initial), want)
    assert (want > initial).all() and not np.array_equal(want, want_counts(parts[:1], bounds, initial))


def test_refusals_write_nothing(built):
    from silo_amd import binding

    n, row_words = 65, 2
    columns = make_columns(n, row_words, 2)
    values_dev = binding._upload(columns)
    out = binding.device_malloc((row_words + GUARD_WORDS) * 8, FILL)
    try:
        good = dict(values_ptr=values_dev, row_words=row_words, sequence_count=n, at_least=0, at_most=NO_BOUND, out_ptr=out)
        for change in (dict(values_ptr=None), dict(out_ptr=None), dict(row_words=0), dict(sequence_count=0), dict(sequence_count=row_words * 64 + 1),
                       dict(sequence_count=NO_BOUND)):
            with pytest.raises(binding.SiloGpuError):
                binding.bitset_from_values_call(**{**good, **change})
        bounds = np.array([(0, NO_BOUND), (0, 5)], dtype=np.uint32)
        counting = dict(values_ptr=values_dev, n_columns=2, row_words=row_words, sequence_count=n, filter_ptr=None, bounds=bounds, counts_ptr=out)
        for change in (dict(values_ptr=None), dict(counts_ptr=None), dict(bounds=None), dict(n_columns=0), dict(n_columns=ref.MAX_REGIONS + 1),
                       dict(row_words=0), dict(sequence_count=0), dict(sequence_count=row_words * 64 + 1)):
            with pytest.raises(binding.SiloGpuError):
                binding.count_values_call(**{**counting, **change})
        assert (binding.device_read(out, np.uint8, (row_words + GUARD_WORDS) * 8) == FILL).all()
        binding.bitset_from_values_call(**good)  # the same buffers serve a good call
        got = binding.device_read(out, np.uint64, row_words + GUARD_WORDS)
        assert np.array_equal(got[:row_words], ref.bitset_words(np.ones(n, dtype=bool), row_words)) and np.array_equal(got[row_words:], GUARD)
    finally:
        binding.device_free(values_dev)
        binding.device_free(out)
