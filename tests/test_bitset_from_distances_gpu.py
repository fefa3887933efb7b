"""silo_gpu_bitset_from_distances (K11's third entry, the leaf of the filter expression WithinDistance) alone, on tables made in
numpy: bit r of the output is r < sequence_count and distance[r] <= max_distance and compared[r] >= min_compared.  The expected
words are np.packbits of that predicate; every comparison is an exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD_WORDS = 4
GUARD = np.full(GUARD_WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
NO_BOUND = 0xFFFFFFFF
SIZES = [1, 63, 64, 65, 255, 256, 257, 2049, 70_001]
PADDING = (0, 0xFFFFFFFF)  # a padding row that would pass any bound


def _row_words(n, rounded):
    words = (n + 63) // 64
    return (words + 31) // 32 * 32 if rounded else words


def _table(n, row_words, seed=0):
    """uint32 [row_words * 64][2]: distances in [0, 40) and compared in [0, 48) for the n rows, PADDING behind them."""
    rng = np.random.default_rng(1000 + seed + n)
    table = np.empty((row_words * 64, 2), dtype=np.uint32)
    table[:] = PADDING
    table[:n, 0] = rng.integers(0, 40, size=n)
    table[:n, 1] = rng.integers(0, 48, size=n)
    return table


def _selected(table, n, max_distance, min_compared):
    rows = np.arange(len(table))
    return (rows < n) & (table[:, 0].astype(np.uint64) <= max_distance) & (table[:, 1].astype(np.uint64) >= min_compared)


def _words(selected):
    return np.packbits(selected, bitorder="little").view(np.uint64)


def _run(table, n, row_words, max_distance=NO_BOUND, min_compared=0):
    from silo_amd import binding

    out = binding.bitset_from_distances(table, n, row_words, max_distance, min_compared, fill=FILL, guard_words=GUARD_WORDS)
    assert np.array_equal(out[row_words:], GUARD), "words past row_words were touched"
    return out[:row_words]


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_word_is_written_and_padding_rows_are_clear(built, n, rounded):
    row_words = _row_words(n, rounded)
    table = _table(n, row_words)
    for max_distance, min_compared in ((NO_BOUND, 0), (7, 0), (39, 30)):
        want = _words(_selected(table, n, max_distance, min_compared))
        assert len(want) == row_words
        got = _run(table, n, row_words, max_distance, min_compared)
        assert np.array_equal(got, want), (n, row_words, max_distance, min_compared)
    # without bounds: exactly the n real rows, although every padding row of the table passes
    everything = _run(table, n, row_words)
    assert int(sum(bin(int(word)).count("1") for word in everything)) == n
    if n % 64:
        assert int(everything[n // 64]) >> (n % 64) == 0
    assert not everything[(n + 63) // 64:].any()


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
def test_bounds(built, rounded):
    n = 70_001
    row_words = _row_words(n, rounded)
    table = _table(n, row_words)
    counts = {}
    for max_distance in (0, 7, 39, 40, NO_BOUND):
        for min_compared in (0, 1, 30, 48, NO_BOUND):
            selected = _selected(table, n, max_distance, min_compared)
            counts[max_distance, min_compared] = int(selected.sum())
            assert np.array_equal(_run(table, n, row_words, max_distance, min_compared), _words(selected)), (max_distance, min_compared)
    # not vacuous, on the numpy side
    assert 0 < counts[7, 0] < n
    assert 0 < counts[39, 30] < n
    assert counts[0, NO_BOUND] == 0
    assert counts[NO_BOUND, 0] == n == counts[40, 0] == counts[39, 0]
    assert counts[NO_BOUND, 48] == 0 and 0 < counts[NO_BOUND, 1] < n


def test_large_values_compare_unsigned(built):
    n = 300
    row_words = _row_words(n, False)
    rng = np.random.default_rng(7)
    table = np.empty((row_words * 64, 2), dtype=np.uint32)
    table[:] = PADDING
    values = np.array([0, 1, 0xFFFF, 0x10000, 0x10001, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    table[:n, 0] = rng.choice(values, size=n)
    table[:n, 1] = rng.choice(values, size=n)
    for max_distance in (0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, NO_BOUND):
        for min_compared in (0, 0x10000, 0x10001, 0x80000000, 0x80000001, NO_BOUND):
            selected = _selected(table, n, max_distance, min_compared)
            assert np.array_equal(_run(table, n, row_words, max_distance, min_compared), _words(selected)), (max_distance, min_compared)
    assert 0 < int(_selected(table, n, 0x80000000, 0x80000000).sum()) < n


def test_a_table_of_zeros(built):
    """Rows with nothing to compare are at distance 0: only min_compared keeps them out."""
    n = 257
    row_words = _row_words(n, False)
    table = np.zeros((row_words * 64, 2), dtype=np.uint32)
    want = _words(np.arange(row_words * 64) < n)
    assert np.array_equal(_run(table, n, row_words, 0, 0), want)
    assert np.array_equal(_run(table, n, row_words, NO_BOUND, 0), want)
    assert not _run(table, n, row_words, 0, 1).any()
    assert not _run(table, n, row_words, NO_BOUND, 1).any()


def test_two_runs_give_the_same_words(built):
    n = 70_001
    row_words = _row_words(n, True)
    table = _table(n, row_words, seed=5)
    first = _run(table, n, row_words, 7, 20)
    second = _run(table, n, row_words, 7, 20)
    assert np.array_equal(first, second) and first.any()


def test_refusals_write_nothing(built):
    from silo_amd import binding

    n, row_words = 65, 2
    table = _table(n, row_words)
    table_dev = binding.device_malloc(table.nbytes)
    out = binding.device_malloc((row_words + GUARD_WORDS) * 8, FILL)
    try:
        binding._check(binding.load_library().silo_gpu_memcpy_h2d(table_dev, binding._ptr(table), table.nbytes, None))
        good = dict(table_ptr=table_dev, sequence_count=n, row_words=row_words, max_distance=NO_BOUND, min_compared=0, out_ptr=out)
        for change in (dict(table_ptr=None), dict(out_ptr=None), dict(row_words=0), dict(sequence_count=0), dict(sequence_count=row_words * 64 + 1),
                       dict(sequence_count=NO_BOUND)):
            with pytest.raises(binding.SiloGpuError):
                binding.bitset_from_distances_call(**{**good, **change})
        assert (binding.device_read(out, np.uint8, (row_words + GUARD_WORDS) * 8) == FILL).all()
        binding.bitset_from_distances_call(**good)  # the same buffers serve a good call
        got = binding.device_read(out, np.uint64, row_words + GUARD_WORDS)
        assert np.array_equal(got[:row_words], _words(np.arange(row_words * 64) < n)) and np.array_equal(got[row_words:], GUARD)
        binding.bitset_from_distances_call(**{**good, "sequence_count": row_words * 64})  # every row of the table is a real row
        assert np.array_equal(binding.device_read(out, np.uint64, row_words), _words(_selected(table, row_words * 64, NO_BOUND, 0)))
    finally:
        binding.device_free(table_dev)
        binding.device_free(out)
