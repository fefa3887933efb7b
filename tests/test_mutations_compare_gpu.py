"""The comparison of count tables (K17, csrc/silo_gpu_compare.hip) through silo_gpu_mutations_compare, on numpy count tables against
tests/mutations_comparison_reference.py (pinned against a plain loop and hand-made rows without a GPU by
tests/test_mutations_comparison_reference.py).

Every comparison is an exact equality.  The output is filled with 0xA5 bytes before the launch and has 16 guard bytes behind it, which
must still hold 0xA5 afterwards, as must every record slot and cell at or past the number of selected cells.  The device's list is
unordered: the records are put in ascending order with their cells before they are compared.  Position counts stand around a wave and
around the 256 positions of a block (where a block's slab of a table starts off a 16-byte boundary), 4 103 gives 17 blocks; 9 tables
are more than a scan batch, 64 the limit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.consensus_reference import VALID  # noqa: E402
from tests.mutations_comparison_reference import HAND_MADE, HEADER_WORDS, MAX_TABLES, THREADS, compare_tables, unpack  # noqa: E402
from tests.test_mutations_comparison_reference import _reference_index, _skewed  # noqa: E402

FILL = 0xA5
SENTINEL = 0xA5A5A5A5
GUARD = 16
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
POSITIONS = [1, 63, 64, 65, 255, 256, 257, 4103]
TABLES = [2, 3, 9, 64]
SETTINGS = [(0.05, 0.0), (0.05, 0.5), (0.5, 0.0), (1.0, 0.0), (0.0, 0.0), (0.05, 0.25), (0.3, 0.1)]


def _check(alphabet, counts, reference_index, min_proportion, min_difference, capacity=None, calls=1):
    """(records, cells) as the device leaves them, in ascending order, after the comparison with the reference.  capacity: None = two
    more than the reference selects."""
    from silo_amd import binding

    tables = counts.shape[0]
    want_records, want_cells, _, _ = compare_tables(counts, reference_index, min_proportion, min_difference)
    selected = len(want_records)
    capacity = selected + 2 if capacity is None else capacity
    out, status = binding.mutations_compare(alphabet, counts, reference_index, min_proportion, min_difference, capacity, fill=FILL, guard_bytes=GUARD, calls=calls)
    case = (alphabet, counts.shape, min_proportion, min_difference, capacity)
    assert status == 0, case
    assert len(out) == HEADER_WORDS + capacity * 2 + capacity * tables * 2 + GUARD // 4
    assert (out[-GUARD // 4:] == SENTINEL).all(), "the guard bytes were written"
    assert out[:HEADER_WORDS].tolist() == [selected, 0, 0, 0], case  # exact, also above the capacity
    fit = min(selected, capacity)
    assert (out[HEADER_WORDS + 2 * fit:HEADER_WORDS + 2 * capacity] == SENTINEL).all(), "a record slot nobody took was written"
    assert (out[HEADER_WORDS + 2 * capacity + 2 * tables * fit:-GUARD // 4] == SENTINEL).all(), "the cells of a slot nobody took were written"
    got_selected, records, cells = unpack(out, tables, capacity)
    assert got_selected == selected
    if fit == selected:
        assert np.array_equal(records, want_records), (case, records[:5], want_records[:5])
        assert np.array_equal(cells, want_cells), (case, np.argwhere(cells != want_cells)[:5])
    else:  # which records found a slot is the device's business: distinct ones of the reference's, with their own cells
        keys = records[:, 0].astype(np.int64) * 32 + records[:, 1]
        want_keys = want_records[:, 0].astype(np.int64) * 32 + want_records[:, 1]
        assert len(set(keys.tolist())) == fit and np.isin(keys, want_keys).all(), case
        assert np.array_equal(cells, want_cells[np.searchsorted(want_keys, keys)]), case
    return records, cells


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.COMPARE_THREADS, binding.MAX_COMPARISON_TABLES, binding.COMPARE_HEADER_WORDS) == (THREADS, MAX_TABLES, HEADER_WORDS) == (256, 64, 4)
    assert {THREADS - 1, THREADS, THREADS + 1} <= set(POSITIONS) and max(POSITIONS) > 16 * THREADS and {2, 9, MAX_TABLES} <= set(TABLES)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("positions", POSITIONS)
def test_shapes(built, alphabet, tables, positions):
    rng = np.random.default_rng(9500 + 10 * positions + tables + (alphabet == "aa"))
    counts = _skewed(rng, alphabet, tables, positions)
    reference_index = _reference_index(rng, alphabet, positions)
    first = (positions + tables) % len(SETTINGS)
    _check(alphabet, counts, reference_index, *SETTINGS[first])
    _check(alphabet, counts, reference_index, *SETTINGS[(first + 3) % len(SETTINGS)])
    everything, _ = _check(alphabet, counts, reference_index, 0.0, 0.0)
    spread, _ = _check(alphabet, counts, reference_index, 0.05, 0.5)
    if positions >= 4000:
        assert 0 < len(spread) < len(everything)  # the settings decide something
        assert everything[0, 0] < THREADS and everything[-1, 0] >= positions - THREADS  # records of the first block and of the last


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_hand_made_rows_at_the_ends_of_a_block_and_in_the_last_table(built, alphabet):
    """Each hand-made position at the first and last position of a block and of the tables; its two or three tables are the LAST of
    five, under tables that are empty there."""
    tables, positions = 5, 2 * THREADS + 7
    places = [0, THREADS - 1, THREADS, 2 * THREADS - 1, 2 * THREADS, positions - 1]
    rng = np.random.default_rng(9600)
    background = _skewed(rng, alphabet, tables, positions)
    background_index = _reference_index(rng, alphabet, positions)
    for what, rows, reference, min_proportion, min_difference, expected in HAND_MADE:
        counts = background.copy()
        reference_index = background_index.copy()
        for position in places:
            counts[:, position] = 0
            counts[tables - len(rows):, position, :5] = np.array(rows, dtype=np.uint32)  # (the rule does not ask which symbols they are)
            reference_index[position] = reference
        records, cells = _check(alphabet, counts, reference_index, min_proportion, min_difference)
        for position in places:
            here = records[:, 0] == position
            assert records[here, 1].tolist() == sorted(expected), (what, position)
            assert cells[here][:, :tables - len(rows)].sum() == 0 and cells[here][:, tables - 1, 0].tolist() == [rows[-1][s] for s in sorted(expected)], what


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_a_capacity_below_the_selected_count(built, alphabet):
    rng = np.random.default_rng(9700)
    counts = _skewed(rng, alphabet, 3, 3 * THREADS + 11)
    reference_index = _reference_index(rng, alphabet, counts.shape[1])
    selected = len(compare_tables(counts, reference_index, 0.05, 0.0)[0])
    assert selected > 600
    for capacity in (selected - 1, 300, 1, 0):
        records, _ = _check(alphabet, counts, reference_index, 0.05, 0.0, capacity=capacity)
        assert len(records) == capacity
    _check(alphabet, counts, reference_index, 0.05, 0.0, capacity=selected)  # exactly as many: what a second call of the host is given


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_a_second_call_gives_the_same_bytes(built, alphabet):
    rng = np.random.default_rng(9800)
    counts = _skewed(rng, alphabet, 5, 3 * THREADS + 11)
    reference_index = _reference_index(rng, alphabet, counts.shape[1])
    once = _check(alphabet, counts, reference_index, 0.05, 0.1)
    twice = _check(alphabet, counts, reference_index, 0.05, 0.1, calls=2)  # (compared with the reference again: the counter is not doubled)
    assert np.array_equal(once[0], twice[0]) and np.array_equal(once[1], twice[1]) and len(once[0]) > 0


def test_refusals_leave_the_fill(built):
    from silo_amd import binding

    rng = np.random.default_rng(9900)
    counts = _skewed(rng, "nuc", 2, 70)
    reference_index = _reference_index(rng, "nuc", 70)

    def refused(alphabet=0, table=counts, min_proportion=0.05, min_difference=0.0, null=(), n_tables=None):
        out, status = binding.mutations_compare(alphabet, table, reference_index, min_proportion, min_difference, 8, fill=FILL, guard_bytes=GUARD, null=null,
                                                n_tables=n_tables)
        assert status == INVALID_ARGUMENT, (alphabet, table.shape, min_proportion, min_difference, null, n_tables)
        assert (out == SENTINEL).all()

    for value in (-0.5, -1e-300, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        refused(min_proportion=value)
        refused(min_difference=value)
    for alphabet in (2, -1):
        refused(alphabet=alphabet)
    refused(table=np.zeros((MAX_TABLES + 1, 70, 5), dtype=np.uint32))
    for n_tables in (0, 1):
        refused(n_tables=n_tables)
    for name in ("counts", "reference", "out"):
        refused(null=(name,))
    assert "mutations_compare" in binding.load_library().silo_gpu_last_error().decode()


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_no_positions(built, alphabet):
    from silo_amd import binding

    counts = np.zeros((3, 0, len(VALID[alphabet])), dtype=np.uint32)
    out, status = binding.mutations_compare(alphabet, counts, np.zeros(0, dtype=np.uint8), 0.05, 0.0, 4, fill=FILL, guard_bytes=GUARD)
    assert status == 0
    assert out[:HEADER_WORDS].tolist() == [0, 0, 0, 0] and (out[HEADER_WORDS:] == SENTINEL).all(), "only the header is cleared"
