"""The consensus call (K15, csrc/silo_gpu_consensus.hip) through silo_gpu_consensus_call, on numpy count tables against
tests/consensus_reference.py (pinned against a character double loop and hand-made rows without a GPU by
tests/test_consensus_reference.py).

Every comparison is an exact equality.  The characters and the summaries are filled with 0xA5 bytes before the launch and have 16
guard bytes behind them, which must still hold 0xA5 afterwards.  Position counts stand around a wave and around the 256 positions
of a block (where a block's slab of the table starts off a 16-byte boundary), 4 103 gives 17 blocks a table.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.consensus_reference import AMBIGUOUS, DELETED, HAND_MADE, LOW_COVERAGE, MAX_TABLES, THREADS, VALID, call_consensus  # noqa: E402

FILL = 0xA5
SENTINEL = 0xA5A5A5A5
GUARD = 16
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
POSITIONS = [1, 63, 64, 65, 255, 256, 257, 4103]
TABLES = [1, 3, 64]


def _check(alphabet, counts, reference_index, threshold, min_depth, calls=1):
    """(chars uint8 [T][P], summary uint32 [T][4]) as the device leaves them, after the comparison with the reference."""
    from silo_amd import binding

    tables, positions = counts.shape[:2]
    chars, summary, status = binding.consensus_call(alphabet, counts, reference_index, threshold, min_depth, fill=FILL, guard_bytes=GUARD, calls=calls)
    assert status == 0
    assert len(chars) == tables * positions + GUARD and len(summary) == tables * 4 + GUARD // 4
    assert (chars[tables * positions:] == FILL).all() and (summary[tables * 4:] == SENTINEL).all(), "the guard bytes were written"
    want_chars, want_summary = call_consensus(counts, reference_index, alphabet, threshold, min_depth)
    chars, summary = chars[:tables * positions].reshape(tables, positions), summary[:tables * 4].reshape(tables, 4)
    assert np.array_equal(summary, want_summary), (alphabet, tables, positions, threshold, min_depth, summary[:4], want_summary[:4])
    assert np.array_equal(chars, want_chars), (alphabet, tables, positions, threshold, min_depth, np.argwhere(chars != want_chars)[:5])
    return chars, summary


def _skewed(rng, alphabet, tables, positions):
    """Count tables with one heavy symbol at most positions, two or three near-equal ones at others, shallow and empty positions."""
    n_symbols = len(VALID[alphabet])
    counts = rng.integers(0, 4, size=(tables, positions, n_symbols)).astype(np.uint32)
    counts[rng.random(counts.shape) < 0.6] = 0
    heavy = rng.integers(0, n_symbols, size=(tables, positions))
    weight = rng.choice(np.array([0, 3, 40, 1000], dtype=np.uint32), size=(tables, positions), p=[0.1, 0.3, 0.3, 0.3])
    np.put_along_axis(counts, heavy[..., None], np.take_along_axis(counts, heavy[..., None], axis=-1) + weight[..., None], axis=-1)
    second = rng.integers(0, n_symbols, size=(tables, positions))
    tied = rng.random((tables, positions)) < 0.2  # a second symbol as heavy as the first, or nearly
    bump = np.where(tied, weight - np.minimum(weight, rng.integers(0, 2, size=weight.shape).astype(np.uint32)), 0).astype(np.uint32)
    np.put_along_axis(counts, second[..., None], np.take_along_axis(counts, second[..., None], axis=-1) + bump[..., None], axis=-1)
    counts[rng.random((tables, positions)) < 0.05] = 0
    return counts


def _reference_index(rng, alphabet, positions):
    index = rng.integers(0, len(VALID[alphabet]), size=positions).astype(np.uint8)
    index[rng.random(positions) < 0.1] = 0xFF
    return index


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.CONSENSUS_THREADS, binding.MAX_CONSENSUS_TABLES, binding.CONSENSUS_SUMMARY_WORDS) == (THREADS, MAX_TABLES, 4) == (256, 64, 4)
    assert {THREADS - 1, THREADS, THREADS + 1} <= set(POSITIONS) and max(POSITIONS) > 16 * THREADS and MAX_TABLES in TABLES


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("positions", POSITIONS)
def test_shapes(built, alphabet, tables, positions):
    rng = np.random.default_rng(9100 + 10 * positions + tables + (alphabet == "aa"))
    counts = _skewed(rng, alphabet, tables, positions)
    reference_index = _reference_index(rng, alphabet, positions)
    threshold, min_depth = [(0.5, 1), (0.75, 3), (0.9, 1), (1.0, 40), (1e-9, 2)][(positions + tables) % 5]
    _, summary = _check(alphabet, counts, reference_index, threshold, min_depth)
    if positions >= 4000:
        assert (summary > 0).all()  # every kind of position occurs in every table
    _check(alphabet, counts, reference_index, 0.75, 1)


def _hand_made(alphabet):
    return [row for row in HAND_MADE if row[0] == alphabet]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_hand_made_rows_at_the_ends_of_a_block_and_of_the_last_table(built, alphabet):
    tables, positions = 3, 2 * THREADS + 7
    places = [(0, 0), (0, THREADS - 1), (0, THREADS), (tables - 1, 2 * THREADS - 1), (tables - 1, 2 * THREADS), (tables - 1, positions - 1)]
    rng = np.random.default_rng(9200)
    background = _skewed(rng, alphabet, tables, positions)
    reference_index = _reference_index(rng, alphabet, positions)
    for _, row, threshold, min_depth, call, kind in _hand_made(alphabet):
        counts = background.copy()
        for table, position in places:
            counts[table, position] = np.array(row, dtype=np.uint32)
        chars, _ = _check(alphabet, counts, reference_index, threshold, min_depth)
        assert all(chr(chars[table, position]) == call for table, position in places), (row, threshold, min_depth, call, kind)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_one_cell_holds_the_highest_count(built, alphabet):
    n_symbols = len(VALID[alphabet])
    positions = n_symbols * 3 + 1
    counts = np.zeros((2, positions, n_symbols), dtype=np.uint32)
    for position in range(positions - 1):
        counts[:, position, position % n_symbols] = 2**32 - 1
    reference_index = (np.arange(positions) % 2).astype(np.uint8)
    for threshold, min_depth in ((1.0, 1), (0.5, 2**32 - 1), (1e-9, 1)):
        chars, summary = _check(alphabet, counts, reference_index, threshold, min_depth)
        assert bytes(chars[1, :n_symbols]).decode("latin-1") == VALID[alphabet]
        assert summary[0, AMBIGUOUS] == 0 and summary[0, LOW_COVERAGE] == 1 and summary[0, DELETED] == 3


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_a_second_call_gives_the_same_bytes(built, alphabet):
    rng = np.random.default_rng(9300)
    counts = _skewed(rng, alphabet, 5, 3 * THREADS + 11)
    reference_index = _reference_index(rng, alphabet, counts.shape[1])
    once = _check(alphabet, counts, reference_index, 0.75, 2)
    twice = _check(alphabet, counts, reference_index, 0.75, 2, calls=2)  # (compared with the reference again: the summary is not doubled)
    assert np.array_equal(once[0], twice[0]) and np.array_equal(once[1], twice[1]) and once[1].sum() > 0


def test_refusals_leave_the_fill(built):
    from silo_amd import binding

    rng = np.random.default_rng(9400)
    counts = _skewed(rng, "nuc", 2, 70)
    reference_index = _reference_index(rng, "nuc", 70)

    def refused(alphabet=0, table=counts, threshold=0.5, min_depth=1, null=()):
        chars, summary, status = binding.consensus_call(alphabet, table, reference_index, threshold, min_depth, fill=FILL, guard_bytes=GUARD, null=null)
        assert status == INVALID_ARGUMENT, (alphabet, table.shape, threshold, min_depth, null)
        assert (chars == FILL).all() and (summary == SENTINEL).all()

    for threshold in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        refused(threshold=threshold)
    refused(min_depth=0)
    for alphabet in (2, -1):
        refused(alphabet=alphabet)
    refused(table=np.zeros((MAX_TABLES + 1, 70, 5), dtype=np.uint32))
    for name in ("counts", "reference", "chars", "summary"):
        refused(null=(name,))
    assert "consensus" in binding.load_library().silo_gpu_last_error().decode()


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_no_positions_and_no_tables(built, alphabet):
    from silo_amd import binding

    n_symbols = len(VALID[alphabet])
    for shape in ((3, 0, n_symbols), (0, 9, n_symbols), (0, 0, n_symbols)):
        chars, summary, status = binding.consensus_call(alphabet, np.zeros(shape, dtype=np.uint32), np.zeros(shape[1], dtype=np.uint8), 0.5, 1, fill=FILL, guard_bytes=GUARD)
        assert status == 0
        assert (chars == FILL).all() and (summary == SENTINEL).all(), "nothing is written where there is nothing to call"
