"""Each row's differences from the reference (K18, csrc/silo_gpu_differences.hip) through silo_gpu_sequence_differences, on numpy
characters against tests/sequence_differences_reference.py (pinned against a plain loop and hand-made rows without a GPU by
tests/test_sequence_differences_reference.py).

Every comparison is an exact equality.  The three outputs are filled with 0xA5 bytes before the launch and have 16 guard bytes behind
each, which must still hold 0xA5 afterwards, as must every record word at or past min(total, capacity).  Position counts stand around
the 16 bytes of a thread, the 1 024 bytes of a wave and the 4 096 bytes of a block's chunk — a chunk is counted from the 16-byte
boundary at or below the row's first byte, so a row of 4 081 positions has one or two chunks and one of 4 082 always two —; they are
mostly odd and the first row starts at every offset from a boundary, so the rows start at every alignment."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.sequence_differences_reference import (CHUNK, DELETION, HAND_MADE, MAX_POSITIONS, MAX_ROWS, MISSING, MISSING_SYMBOL, QUAD, STATS, WAVE_BYTES,  # noqa: E402
                                                  classify, difference_records, hand_made_matrix, skewed_chars)

FILL = 0xA5
SENTINEL = 0xA5A5A5A5
GUARD = 16
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
POSITIONS = [1, 15, 16, 17, 1023, 1025, 4081, 4082, 4095, 4096, 4097, 8193]
ROWS = [1, 2, 3, 65]


def _check(alphabet, chars, reference, capacity=None, calls=1, chars_offset=0):
    """(offsets, stats, words) as the device leaves them, after the comparison with the reference.  capacity: None = two more than
    the reference's total."""
    from silo_amd import binding

    n = chars.shape[0]
    want_offsets, want_stats, want_words = difference_records(chars, reference, alphabet)
    total = len(want_words)
    capacity = total + 2 if capacity is None else capacity
    offsets, stats, records, status = binding.sequence_differences(alphabet, chars, reference, capacity, fill=FILL, guard_bytes=GUARD, calls=calls,
                                                                   chars_offset=chars_offset)
    case = (alphabet, chars.shape, capacity, calls, chars_offset)
    assert status == 0, case
    guard = GUARD // 4
    assert len(offsets) == n + 1 + guard and len(stats) == n * STATS + guard and len(records) == capacity + guard
    for out in (offsets, stats, records):
        assert (out[-guard:] == SENTINEL).all(), "the guard bytes were written"
    assert np.array_equal(offsets[:n + 1], want_offsets), (case, np.flatnonzero(offsets[:n + 1] != want_offsets)[:5])  # exact, also above the capacity
    assert np.array_equal(stats[:n * STATS].reshape(n, STATS), want_stats), (case, np.argwhere(stats[:n * STATS].reshape(n, STATS) != want_stats)[:5])
    fit = min(total, capacity)
    wrong = np.flatnonzero(records[:fit] != want_words[:fit])
    assert len(wrong) == 0, (case, wrong[:5], records[wrong[:5]], want_words[wrong[:5]])
    assert (records[fit:capacity] == SENTINEL).all(), "a word at or past min(total, capacity) was written"
    return offsets[:n + 1], stats[:n * STATS], records[:fit]


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.DIFFERENCE_CHUNK, binding.DIFFERENCE_STATS, binding.MAX_DIFFERENCE_ROWS, binding.MAX_DIFFERENCE_POSITIONS) == (CHUNK, STATS, MAX_ROWS, MAX_POSITIONS)
    assert (QUAD, WAVE_BYTES, CHUNK) == (16, 1024, 4096)
    assert {QUAD - 1, QUAD, QUAD + 1, WAVE_BYTES - 1, WAVE_BYTES + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1} <= set(POSITIONS)
    assert {CHUNK - 15, CHUNK - 14} <= set(POSITIONS)  # the most positions whose row is one chunk at every alignment, and one more
    assert binding.difference_chunks(CHUNK - 15) == 1 and binding.difference_chunks(CHUNK - 14) == 2
    assert sum(p % 2 for p in POSITIONS) >= 8 and {1, 2, 3} <= set(ROWS) and max(ROWS) > 64


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("positions", POSITIONS)
def test_shapes(built, alphabet, rows, positions):
    rng = np.random.default_rng(18_000 + 10 * positions + rows + (alphabet == "aa"))
    chars, reference = skewed_chars(rng, alphabet, rows, positions)
    offsets, stats, words = _check(alphabet, chars, reference, chars_offset=(positions + 5 * rows) % 16)
    if rows * positions >= 60_000:  # not vacuous
        assert 0 < len(words) < rows * positions // 4 and (stats.reshape(rows, STATS).sum(axis=0) > 0).all()
        classes = classify(chars, reference, alphabet)
        assert any(classes[r, -1] == classes[r + 1, 0] and classes[r, -1] in (DELETION, MISSING) for r in range(rows - 1))


@pytest.mark.parametrize("case", range(len(HAND_MADE)))
def test_hand_made_rows(built, case):
    what, alphabet = HAND_MADE[case][:2]
    chars, reference, want = hand_made_matrix(HAND_MADE[case])
    for chars_offset in (0, 9):
        _, _, words = _check(alphabet, chars, reference, chars_offset=chars_offset)
        assert words.tolist() == want.tolist(), what
    # the same cells at the end of rows of 4 099 positions: around the end of the first chunk
    lead = CHUNK + 3 - chars.shape[1]
    filler = np.frombuffer(("ACGT" * (lead // 4 + 1))[:lead].encode(), dtype=np.uint8)
    long_chars = np.concatenate([np.repeat(filler[None, :], len(chars), axis=0), chars], axis=1)
    _, _, words = _check(alphabet, long_chars, np.concatenate([filler, reference]))
    kept = [word for word in want.tolist() if not (word >> 9 == 0 and (word >> 8) & 1)]
    assert [(word >> 9) - lead for word in words.tolist()] == [word >> 9 for word in kept] and [word & 0x1FF for word in words.tolist()] == [word & 0x1FF for word in kept], what


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_runs_across_every_boundary(built, alphabet):
    """Row r holds a run of 20 cells that starts r % 13 cells before each boundary of a thread, a wave and a chunk — rows of odd
    length, so the boundaries fall differently in every row —, of the missing symbol in even rows and of '-' in odd ones, and a
    one-cell run of the other symbol; every row ends in a run and the next begins with the same symbol, which must emit its own
    start."""
    rows, positions = 40, 2 * CHUNK + 37
    rng = np.random.default_rng(18_500)
    chars, reference = skewed_chars(rng, alphabet, rows, positions)
    chars[:] = reference[None, :]
    symbols = (ord(MISSING_SYMBOL[alphabet]), ord("-"))
    for r in range(rows):
        for boundary in (QUAD, WAVE_BYTES, CHUNK, CHUNK + WAVE_BYTES, 2 * CHUNK):
            chars[r, boundary - r % 13:boundary - r % 13 + 20] = symbols[r % 2]
        chars[r, 600 + r] = symbols[1 - r % 2]
        chars[r, -(1 + r % 5):] = symbols[r % 2]
        if r != 0:
            chars[r, :1 + r % 3] = symbols[(r - 1) % 2]  # begins with what the row before ends with
    offsets, _, words = _check(alphabet, chars, reference, chars_offset=3)
    for r in range(1, rows):
        first = int(words[offsets[r]])
        assert first >> 9 == 0 and (first & 0x100) == 0 and (first & 0xFF) == chars[r, 0] == chars[r - 1, -1], r  # its own start


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_a_capacity_below_the_total(built, alphabet):
    rng = np.random.default_rng(18_700)
    chars, reference = skewed_chars(rng, alphabet, 7, CHUNK + 301)
    total = len(difference_records(chars, reference, alphabet)[2])
    assert total > 600
    for capacity in (total - 1, 300, 1, 0):
        _, _, words = _check(alphabet, chars, reference, capacity=capacity)
        assert len(words) == capacity
    _check(alphabet, chars, reference, capacity=total)  # exactly as many: what a second call of the host is given


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_a_second_call_gives_the_same_bytes(built, alphabet):
    rng = np.random.default_rng(18_800)
    chars, reference = skewed_chars(rng, alphabet, 5, CHUNK + 301)
    once = _check(alphabet, chars, reference)
    twice = _check(alphabet, chars, reference, calls=2)
    assert all(np.array_equal(a, b) for a, b in zip(once, twice)) and len(once[2]) > 0
    short = _check(alphabet, chars, reference, capacity=100, calls=2)
    assert np.array_equal(short[2], once[2][:100])


def test_refusals_leave_the_fill(built):
    from silo_amd import binding

    rng = np.random.default_rng(18_900)
    chars, reference = skewed_chars(rng, "nuc", 3, 70)

    def call(alphabet=0, capacity=8, **told):
        return binding.sequence_differences(alphabet, chars, reference, capacity, fill=FILL, guard_bytes=GUARD, **told)

    def refused(**told):
        offsets, stats, records, status = call(**told)
        assert status == INVALID_ARGUMENT, told
        assert (offsets == SENTINEL).all() and (stats == SENTINEL).all() and (records == SENTINEL).all(), told

    for alphabet in (2, -1):
        refused(alphabet=alphabet)
    for name in ("chars", "reference", "offsets", "stats", "records", "scratch"):
        refused(null=(name,))
    refused(n_rows=MAX_ROWS + 1)
    refused(positions=MAX_POSITIONS + 1)
    refused(n_rows=1 << 10, positions=1 << 22)  # 2^32 characters
    refused(n_rows=MAX_ROWS, positions=MAX_POSITIONS)
    assert "sequence_differences" in binding.load_library().silo_gpu_last_error().decode()
    offsets, stats, records, status = call(capacity=0, null=("records",))  # no list asked for: no list needed
    want_offsets, want_stats, _ = difference_records(chars, reference, "nuc")
    assert status == 0 and np.array_equal(offsets[:4], want_offsets) and np.array_equal(stats[:12].reshape(3, STATS), want_stats)
    assert (records == SENTINEL).all() and (offsets[4:] == SENTINEL).all() and (stats[12:] == SENTINEL).all()


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_no_rows_and_no_positions(built, alphabet):
    from silo_amd import binding

    reference = np.frombuffer(b"ACGTA", dtype=np.uint8)
    offsets, stats, records, status = binding.sequence_differences(alphabet, np.zeros((0, 5), dtype=np.uint8), reference, 4, fill=FILL, guard_bytes=GUARD)
    assert status == 0 and offsets[0] == 0 and (offsets[1:] == SENTINEL).all() and (stats == SENTINEL).all() and (records == SENTINEL).all()
    offsets, stats, records, status = binding.sequence_differences(alphabet, np.zeros((3, 0), dtype=np.uint8), reference[:0], 4, fill=FILL, guard_bytes=GUARD)
    assert status == 0 and offsets[:4].tolist() == [0, 0, 0, 0] and (offsets[4:] == SENTINEL).all()
    assert not stats[:12].any() and (stats[12:] == SENTINEL).all() and (records == SENTINEL).all()
