"""silo_gpu_bitset_from_cell_counts (K22, the leaf of the filter expression CellCount) alone, on tables made in numpy: bit r of the
output is r < sequence_count and at_least <= value(r) <= at_most, value(r) the 64-bit sum of the kinds of the mask.  The expected
words are np.packbits of that predicate (tests/cell_counts_reference.py); every comparison is an exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cell_counts_reference as ref  # noqa: E402

FILL = 0xA5
GUARD_WORDS = 4
GUARD = np.full(GUARD_WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
NO_BOUND = 0xFFFFFFFF
SIZES = [1, 63, 64, 65, 255, 256, 257, 2049, 70_001]
MASKS = [1, 2, 4, 8, 5, 10, 15]  # every single kind, two pairs, all four
PADDING = 0xFFFFFFFF            # the cells of a padding row


def row_words_of(n, rounded):
    words = (n + 63) // 64
    return (words + 31) // 32 * 32 if rounded else words


def make_table(n, row_words, seed=0):
    """uint32 [row_words * 64][4]: substitutions in [0, 40), deletions in [0, 12), missing in [0, 300) (a third of the rows 0),
    ambiguous in [0, 5) for the n rows, PADDING behind them."""
    rng = np.random.default_rng(3000 + seed + n)
    table = np.full((row_words * 64, 4), PADDING, dtype=np.uint32)
    table[:n, 0] = rng.integers(0, 40, size=n)
    table[:n, 1] = rng.integers(0, 12, size=n)
    table[:n, 2] = rng.integers(0, 300, size=n) * (rng.random(n) > 0.33)
    table[:n, 3] = rng.integers(0, 5, size=n)
    return table


def bounds_of(table, n, mask):
    """(at_least, at_most) pairs at, one below and one above values present, with 0, UINT32_MAX and an empty interval."""
    present = np.unique(ref.values(table[:n], mask))
    middle = int(present[len(present) // 2])
    return [(0, NO_BOUND), (0, middle), (middle, NO_BOUND), (middle, middle), (max(middle - 1, 0), middle + 1), (middle + 1, NO_BOUND),
            (0, max(middle - 1, 0)), (int(present[-1]), NO_BOUND), (int(present[-1]) + 1, NO_BOUND), (0, 0), (NO_BOUND, NO_BOUND), (middle + 1, middle)]


def words_of(selected):
    return np.packbits(selected, bitorder="little").view(np.uint64)


def _run(table, n, row_words, mask, at_least=0, at_most=NO_BOUND):
    from silo_amd import binding

    out = binding.bitset_from_cell_counts(table, row_words, n, mask, at_least, at_most, fill=FILL, guard_words=GUARD_WORDS)
    assert np.array_equal(out[row_words:], GUARD), "words past row_words were touched"
    return out[:row_words]


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_word_is_written_and_padding_rows_are_clear(built, n, rounded):
    row_words = row_words_of(n, rounded)
    table = make_table(n, row_words)
    for mask, at_least, at_most in ((4, 0, 0), (1, 7, 20), (15, 30, 200)):
        want = words_of(ref.selected(table, n, mask, at_least, at_most))
        assert len(want) == row_words
        assert np.array_equal(_run(table, n, row_words, mask, at_least, at_most), want), (n, row_words, mask, at_least, at_most)
    # without bounds: exactly the n real rows, although every padding row of the table passes
    everything = _run(table, n, row_words, 15)
    assert int(sum(bin(int(word)).count("1") for word in everything)) == n
    if n % 64:
        assert int(everything[n // 64]) >> (n % 64) == 0
    assert not everything[(n + 63) // 64:].any()


@pytest.mark.parametrize("mask", MASKS)
def test_masks_and_bounds(built, mask):
    n = 70_001
    row_words = row_words_of(n, True)
    table = make_table(n, row_words)
    counts = []
    for at_least, at_most in bounds_of(table, n, mask):
        selected = ref.selected(table, n, mask, at_least, at_most)
        counts.append(int(selected.sum()))
        assert np.array_equal(_run(table, n, row_words, mask, at_least, at_most), words_of(selected)), (mask, at_least, at_most)
    # not vacuous, on the numpy side
    assert counts[0] == n and 0 < counts[1] < n and 0 < counts[2] < n and 0 < counts[3] < counts[1]
    assert counts[8] == 0 and counts[10] == 0 and counts[11] == 0 and counts[7] > 0


def test_four_values_near_2_to_the_32_do_not_wrap(built):
    n = 300
    row_words = row_words_of(n, False)
    rng = np.random.default_rng(7)
    big = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    table = np.full((row_words * 64, 4), PADDING, dtype=np.uint32)
    table[:n] = rng.choice(big, size=(n, 4))
    table[0] = 0xFFFFFFFF  # value 4 * (2^32 - 1) under mask 15: wrapped to 32 bits it would be 2^32 - 4
    table[1] = (1, 0xFFFFFFFF, 0, 0)  # wrapped: 0
    for mask in (15, 3, 9, 1):
        for at_least, at_most in ((0, NO_BOUND), (0, 0), (0, 0xFFFFFFFB), (0xFFFFFFFC, NO_BOUND), (NO_BOUND, NO_BOUND), (0x80000000, NO_BOUND), (1, 0x7FFFFFFF)):
            selected = ref.selected(table, n, mask, at_least, at_most)
            assert np.array_equal(_run(table, n, row_words, mask, at_least, at_most), words_of(selected)), (mask, at_least, at_most)
    assert not ref.selected(table, n, 15, 0, NO_BOUND)[0] and not ref.selected(table, n, 3, 0, 0)[1]
    assert 0 < int(ref.selected(table, n, 15, 0, NO_BOUND).sum()) < n


def test_two_runs_give_the_same_words(built):
    n = 70_001
    row_words = row_words_of(n, True)
    table = make_table(n, row_words, seed=5)
    first = _run(table, n, row_words, 5, 10, 150)
    second = _run(table, n, row_words, 5, 10, 150)
    assert np.array_equal(first, second) and first.any()


def test_refusals_write_nothing(built):
    from silo_amd import binding

    n, row_words = 65, 2
    table = make_table(n, row_words)
    table_dev = binding._upload(table)
    out = binding.device_malloc((row_words + GUARD_WORDS) * 8, FILL)
    try:
        good = dict(table_ptr=table_dev, row_words=row_words, sequence_count=n, kinds_mask=15, at_least=0, at_most=NO_BOUND, out_ptr=out)
        for change in (dict(table_ptr=None), dict(out_ptr=None), dict(row_words=0), dict(sequence_count=0), dict(sequence_count=row_words * 64 + 1),
                       dict(sequence_count=NO_BOUND), dict(kinds_mask=0), dict(kinds_mask=16), dict(kinds_mask=NO_BOUND)):
            with pytest.raises(binding.SiloGpuError):
                binding.bitset_from_cell_counts_call(**{**good, **change})
        assert (binding.device_read(out, np.uint8, (row_words + GUARD_WORDS) * 8) == FILL).all()
        binding.bitset_from_cell_counts_call(**good)  # the same buffers serve a good call
        got = binding.device_read(out, np.uint64, row_words + GUARD_WORDS)
        assert np.array_equal(got[:row_words], words_of(np.arange(row_words * 64) < n)) and np.array_equal(got[row_words:], GUARD)
        binding.bitset_from_cell_counts_call(**{**good, "sequence_count": row_words * 64, "at_least": 5})  # every row of the table is a real row
        assert np.array_equal(binding.device_read(out, np.uint64, row_words), words_of(ref.selected(table, row_words * 64, 15, 5, NO_BOUND)))
    finally:
        binding.device_free(table_dev)
        binding.device_free(out)
