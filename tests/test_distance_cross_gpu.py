"""The rectangle kernel of NearestAmong (K14, csrc/silo_gpu_distance.hip) through silo_gpu_distance_cross, against the numpy
reference of tests/neighbours_reference.py (pinned without a GPU by tests/test_neighbours_reference.py).

tests/test_nearest_among_gpu.py reaches it through JSON and the engine.  Here the entry gets the shapes where the kernel takes
another path: rows and columns around the 16 x 64 tile; positions around a word and around the chunk of words a block stages; both
bounds at, below and above values that occur; tiles that stop early, tiles that must not, and an edge tile; every kind of self
column; the same buffer on both sides against silo_gpu_distance_weights, the kernel it shares its walk with; special rows; the
limits; the refusals.  Every case has the cells filled with 0xA5 bytes before the launch and four guard words behind them, and every
comparison is an exact equality.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.neighbours_reference import NOT_ELIGIBLE, cells_of, cross_counts  # noqa: E402
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}
TR = 16   # SILO_GPU_WITHIN_TILE_ROWS: what the row counts below stand around
TC = 64   # SILO_GPU_WITHIN_TILE_COLS: what the column counts below stand around
C = 16    # SILO_GPU_WITHIN_CHUNK_WORDS: what the positions below stand around
FILL = 0xA5
SENTINEL = 0xA5A5A5A5
GUARD = 4
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
LONG = 4103            # positions of the early-exit cases: several chunks
NO_BOUND = NOT_ELIGIBLE


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.WITHIN_TILE_ROWS, binding.WITHIN_TILE_COLS, binding.WITHIN_CHUNK_WORDS) == (TR, TC, C)
    assert (binding.MAX_CROSS_ROWS, binding.MAX_CROSS_COLUMNS) == (2048, 8192)
    assert LONG > 2 * 64 * C and binding.NOT_ELIGIBLE == NOT_ELIGIBLE


def _draw(rng, name, n, positions, changed=0.1):
    """uint8 [n][positions]: one row of valid symbols, copied n times with a share of the positions redrawn from the whole
    alphabet — most positions agree."""
    all_chars, valid_chars = ALPHABETS[name]
    base = rng.choice(np.frombuffer(valid_chars.encode(), dtype=np.uint8), size=positions)
    chars = np.tile(base, (n, 1))
    redrawn = rng.random((n, positions)) < changed
    chars[redrawn] = rng.choice(np.frombuffer(all_chars.encode(), dtype=np.uint8), size=int(redrawn.sum()))
    return chars


class Packed:
    """The planes of both sides on the device, and the reference's two counts per pair: several bounds are asked of one packing."""

    def __init__(self, name, subjects, candidates):
        from silo_amd import binding

        self.name = name
        self.m, self.positions = subjects.shape
        self.n = len(candidates)
        self.rows = binding.distance_pack_rows(name, subjects, fill=FILL)
        self.columns = binding.distance_pack_rows(name, candidates, fill=FILL)
        self.differing, self.compared = cross_counts(subjects, candidates, ALPHABETS[name][1])

    def __enter__(self):
        return self

    def __exit__(self, *_):
        from silo_amd import binding

        binding.device_free(self.rows)
        binding.device_free(self.columns)

    def check(self, max_distance, min_compared, self_columns=None):
        """The cells uint32 [m][n][2] after the checks."""
        from silo_amd import binding

        m, n = self.m, self.n
        out = binding.distance_cross(
            self.name, self.rows, m, self.columns, n, self.positions, self_columns, max_distance, min_compared, fill=FILL, guard_words=GUARD
        )
        assert len(out) == m * n * 2 + GUARD and (out[m * n * 2:] == SENTINEL).all(), "the guard words were written"
        got = out[:m * n * 2].reshape(m, n, 2)
        want = cells_of(self.differing, self.compared, self_columns, max_distance, min_compared)
        assert np.array_equal(got, want), (self.name, m, n, self.positions, max_distance, min_compared, np.argwhere(got != want)[:5])
        return got


def _occurring(packed):
    """(d, c): a distance and a compared count that occur among the pairs, in the middle of what occurs."""
    distances, counts = np.sort(packed.differing.ravel()), np.sort(packed.compared.ravel())
    return int(distances[len(distances) // 2]), int(counts[len(counts) // 2])


def _eligible(cells):
    return int((cells[..., 0] != NOT_ELIGIBLE).sum())


# ---- a: rows and columns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("n", [1, TC - 1, TC, TC + 1, 2 * TC + 1])
@pytest.mark.parametrize("m", [1, TR - 1, TR, TR + 1, 2 * TR + 1])
def test_rows_and_columns_around_the_tile(built, name, m, n):
    assert (1, 15, 16, 17, 33) == (1, TR - 1, TR, TR + 1, 2 * TR + 1) and (1, 63, 64, 65, 129) == (1, TC - 1, TC, TC + 1, 2 * TC + 1)
    rng = np.random.default_rng(5100 + 1000 * m + n)
    chars = _draw(rng, name, m + n, 130, changed=0.05)
    with Packed(name, chars[:m], chars[m:]) as packed:
        d, c = _occurring(packed)
        assert _eligible(packed.check(NO_BOUND, 0)) == m * n
        some = packed.check(d, 0)
        packed.check(d, c, self_columns=np.arange(m, dtype=np.uint32) % n)
        if m * n > 100:
            assert 0 < _eligible(some) < m * n


# ---- b: positions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("positions", [1, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1, LONG])
def test_positions_around_a_word_and_a_chunk(built, name, positions):
    assert (1023, 1024, 1025, 4103) == (64 * C - 1, 64 * C, 64 * C + 1, LONG)
    rng = np.random.default_rng(5200 + positions)
    chars = _draw(rng, name, 100, positions, changed=0.02 if positions > 100 else 0.3)
    with Packed(name, chars[:20], chars[20:]) as packed:
        d, c = _occurring(packed)
        some = packed.check(d, c)
        assert _eligible(packed.check(NO_BOUND, 0)) == 20 * 80
        packed.check(0, 0)
        if positions > 1:
            assert 0 < _eligible(some) < 20 * 80


# ---- c: the two bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_bounds_at_below_and_above_values_that_occur(built, name):
    rng = np.random.default_rng(5300)
    chars = _draw(rng, name, 100, 130, changed=0.08)
    with Packed(name, chars[:20], chars[20:]) as packed:
        d, c = _occurring(packed)
        assert d >= 1 and c >= 1
        eligible = {}
        for max_distance in (0, d - 1, d, NO_BOUND):
            for min_compared in (0, c, c + 1, NO_BOUND):
                eligible[max_distance, min_compared] = _eligible(packed.check(max_distance, min_compared))
        assert eligible[d - 1, 0] < eligible[d, 0] < eligible[NO_BOUND, 0] == 20 * 80     # a pair at exactly d
        assert eligible[NO_BOUND, c + 1] < eligible[NO_BOUND, c] < eligible[NO_BOUND, 0]  # a pair at exactly c
        assert all(count == 0 for (_, min_compared), count in eligible.items() if min_compared == NO_BOUND)


# ---- d: early exit ---------------------------------------------------------------------------------------------------------------
def _prefix(name, shift):
    """64 valid symbols, symbol (position + shift) of the valid ones in a circle: two such prefixes differ at every position unless
    their shifts are equal modulo the number of valid symbols."""
    valid = np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8)
    return valid[(np.arange(64) + shift) % len(valid)]


@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("with_the_pair", [True, False])
def test_a_tile_of_far_pairs_stops_unless_one_pair_is_near(built, name, with_the_pair):
    """16 subjects against 128 candidates: two tiles.  The subjects and the candidates 64 .. 127 differ at every one of the first 64
    positions, so the second tile stops after its first chunk and every one of its cells is the UINT32_MAX pair (not the 0xA5 bytes
    the buffer held) — unless subject 3 and candidate 74 are made equal but for one position of the last word: then the tile must
    walk to the end for that pair, whose differences all lie in the last word."""
    rng = np.random.default_rng(5500)
    chars = _draw(rng, name, TR + 2 * TC, LONG, changed=0.0)
    chars[:TR + TC, :64] = _prefix(name, 0)
    chars[TR + TC:, :64] = _prefix(name, 1)
    tail = rng.random((TR + 2 * TC, LONG - 64)) < 0.0003   # a few differences behind the prefix, within the groups too
    chars[:, 64:][tail] = ord("-")
    subjects, candidates = chars[:TR].copy(), chars[TR:].copy()
    if with_the_pair:
        subjects[3, :64] = candidates[74, :64] = _prefix(name, 2)
        candidates[74, 64:] = subjects[3, 64:]
        candidates[74, LONG - 1] = ord("A") if subjects[3, LONG - 1] != ord("A") else ord("C")
    with Packed(name, subjects, candidates) as packed:
        far = packed.differing[:, TC:]
        if with_the_pair:
            assert far[3, 10] == 1 and np.sort(far.ravel())[1] >= 64
            assert _eligible(packed.check(0, 0)[:, TC:]) == 0
            got = packed.check(5, 0)
            assert got[3, 74].tolist() == [1, int(packed.compared[3, 74])] and _eligible(got[:, TC:]) == 1
        else:
            assert far.min() >= 64
            got = packed.check(5, 0)
            assert (got[:, TC:] == NOT_ELIGIBLE).all() and _eligible(got[:, :TC]) > 0
        assert _eligible(packed.check(NO_BOUND, 0)) == _eligible(packed.check(LONG, 0)) == TR * 2 * TC  # nothing stops


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_an_edge_tile_whose_rows_and_columns_past_the_counts_would_have_distance_zero(built, name):
    """21 subjects against 69 candidates: the tile of rows 16 .. 31 against columns 64 .. 127 holds 5 x 5 pairs that exist — which
    differ at every one of the first 64 positions — and rows past m and columns past n, staged as zeros, whose distance to
    anything is 0: they must neither keep the tile walking into a wrong answer, nor be written."""
    rng = np.random.default_rng(5600)
    m, n = TR + 5, TC + 5
    chars = _draw(rng, name, m + n, LONG, changed=0.0)
    chars[:m, :64] = _prefix(name, 0)
    chars[m:, :64] = _prefix(name, 0)
    chars[m + TC:, :64] = _prefix(name, 1)
    with Packed(name, chars[:m], chars[m:]) as packed:
        assert packed.differing[:, TC:].min() >= 64
        got = packed.check(5, 0)
        assert (got[:, TC:] == NOT_ELIGIBLE).all() and _eligible(got[:, :TC]) == m * TC
        packed.check(0, 0)
        packed.check(64, 0)


# ---- e: self ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_self_columns(built, name):
    """NULL, the first column, the last column, the middle of a tile, a value at or past n, and two subjects naming one column."""
    rng = np.random.default_rng(5700)
    m, n = 20, 150
    chars = _draw(rng, name, m + n, 130, changed=0.05)
    with Packed(name, chars[:m], chars[m:]) as packed:
        assert _eligible(packed.check(NO_BOUND, 0, None)) == m * n
        self_columns = np.full(m, NOT_ELIGIBLE, dtype=np.uint32)
        self_columns[[0, 1, 2, 3, 4, 17, 18]] = [0, n - 1, 100, n, 2**31, 77, 77]
        got = packed.check(NO_BOUND, 0, self_columns)
        assert _eligible(got) == m * n - 5
        for row, column in ((0, 0), (1, n - 1), (2, 100), (17, 77), (18, 77)):
            assert got[row, column].tolist() == [NOT_ELIGIBLE, NOT_ELIGIBLE]
        d, c = _occurring(packed)
        packed.check(d, c, self_columns)
        assert _eligible(packed.check(NO_BOUND, 0, np.full(m, n, dtype=np.uint32))) == m * n


@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("n", [80, 211])
def test_the_same_buffer_on_both_sides_equals_the_weights_kernel(built, name, n):
    from silo_amd import binding

    rng = np.random.default_rng(5800 + n)
    chars = _draw(rng, name, n, 130, changed=0.05)
    planes = binding.distance_pack_rows(name, chars, fill=FILL)
    try:
        differing, compared = cross_counts(chars, chars, ALPHABETS[name][1])
        d, c = int(np.median(differing)), int(np.median(compared))
        for max_distance, min_compared in ((NO_BOUND, 0), (d, 0), (d, c)):
            out = binding.distance_cross(name, planes, n, planes, n, 130, np.arange(n, dtype=np.uint32), max_distance, min_compared, fill=FILL, guard_words=GUARD)
            assert (out[n * n * 2:] == SENTINEL).all()
            cells = out[:n * n * 2].reshape(n, n, 2)
            assert np.array_equal(cells, cells_of(differing, compared, np.arange(n), max_distance, min_compared))
            weights = binding.distance_weights(name, planes, n, 130, max_distance, min_compared, fill=FILL)
            assert np.array_equal(cells[..., 0], weights.reshape(n, n))
    finally:
        binding.device_free(planes)


# ---- f: special rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_special_rows(built, name):
    """Identical rows have distance 0; a row of the missing symbol has (0, 0) against everything, eligible with min_compared 0
    and not with 1; the bytes a, ? and NUL are not valid."""
    all_chars, valid_chars = ALPHABETS[name]
    positions = 150
    rng = np.random.default_rng(5900)
    ordinary = _draw(rng, name, 1, positions, changed=0.3)[0]
    valid = np.frombuffer(valid_chars.encode(), dtype=np.uint8)
    everywhere = valid[np.arange(positions) % len(valid)]
    shifted = valid[(np.arange(positions) + 1) % len(valid)]
    strange = everywhere.copy()
    strange[[0, 64, 149]] = [ord("a"), ord("?"), 0]
    missing = np.full(positions, ord(all_chars[-1]), dtype=np.uint8)
    subjects = np.stack([ordinary, missing, everywhere, strange])
    candidates = np.stack([ordinary, ordinary, missing, everywhere, shifted, strange, missing])
    with Packed(name, subjects, candidates) as packed:
        unbounded = packed.check(NO_BOUND, 0)
        assert unbounded[0, 0, 0] == 0 and unbounded[0, 1, 0] == 0 and (unbounded[1] == 0).all() and (unbounded[:, 2] == 0).all()
        assert unbounded[2, 4].tolist() == [positions, positions] and unbounded[2, 5].tolist() == [0, positions - 3]
        assert unbounded[3, 5].tolist() == [0, positions - 3] and unbounded[3, 4].tolist() == [positions - 3, positions - 3]
        at_one = packed.check(0, 1)
        assert (at_one[1] == NOT_ELIGIBLE).all() and (at_one[:, [2, 6]] == NOT_ELIGIBLE).all() and at_one[0, 0].tolist() == [0, int(packed.compared[0, 0])]
        assert packed.check(0, positions - 3)[2, 5, 0] == 0 and packed.check(0, positions - 2)[2, 5, 0] == NOT_ELIGIBLE
        assert packed.check(positions - 3, 0)[3, 4, 0] == positions - 3 and packed.check(positions - 4, 0)[3, 4, 0] == NOT_ELIGIBLE


# ---- g: large shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,n", [("nuc", 130, 4097), ("aa", 2048, 70)])
def test_large_shapes(built, name, m, n):
    rng = np.random.default_rng(6000 + m)
    kinds = rng.choice(np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8), size=(40, 70))   # 40 kinds of row, far apart ...
    chars = kinds[rng.integers(0, 40, size=m + n)]
    redrawn = rng.random(chars.shape) < 0.01                                                         # ... and near copies of them
    chars[redrawn] = rng.choice(np.frombuffer(ALPHABETS[name][0].encode(), dtype=np.uint8), size=int(redrawn.sum()))
    with Packed(name, chars[:m], chars[m:]) as packed:
        got = packed.check(1, 60, self_columns=(np.arange(m, dtype=np.uint32) * 31) % (n + 5))
        assert 0 < _eligible(got) < m * n // 10 and _eligible(got[-1:]) + _eligible(got[:, -1:]) > 0


# ---- h: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_no_rows_no_columns_and_no_positions(built):
    """2 049 rows, 8 193 columns, an alphabet that does not exist, NULL buffers: SILO_GPU_ERR_INVALID_ARGUMENT and nothing written;
    no rows or no columns: success and nothing written; no positions: the cells of "compared = distance = 0"; the next valid call
    answers exactly."""
    from silo_amd import binding

    lib = binding.load_library()
    rng = np.random.default_rng(6100)
    chars = _draw(rng, "nuc", 20 + 70, 70)
    rows_dev = binding.distance_pack_rows("nuc", chars[:20])
    columns_dev = binding.distance_pack_rows("nuc", chars[20:])
    self_columns = np.full(20, NOT_ELIGIBLE, dtype=np.uint32)
    self_columns[5] = 9
    self_dev = binding.device_malloc(80)
    binding._check(lib.silo_gpu_memcpy_h2d(self_dev, binding._ptr(self_columns), 80, None))
    words = 20 * 70 * 2
    out_dev = binding.device_malloc((words + GUARD) * 4, fill=FILL)
    null = ctypes.c_void_p(0)

    def read():
        return binding.device_read(out_dev, np.uint32, words + GUARD)

    refused = [
        lib.silo_gpu_distance_cross(0, rows_dev, binding.MAX_CROSS_ROWS + 1, columns_dev, 70, 70, self_dev, 3, 0, out_dev, None),
        lib.silo_gpu_distance_cross(0, rows_dev, 20, columns_dev, binding.MAX_CROSS_COLUMNS + 1, 70, self_dev, 3, 0, out_dev, None),
        lib.silo_gpu_distance_cross(2, rows_dev, 20, columns_dev, 70, 70, self_dev, 3, 0, out_dev, None),
        lib.silo_gpu_distance_cross(-1, rows_dev, 20, columns_dev, 70, 70, self_dev, 3, 0, out_dev, None),
        lib.silo_gpu_distance_cross(0, null, 20, columns_dev, 70, 70, self_dev, 3, 0, out_dev, None),
        lib.silo_gpu_distance_cross(0, rows_dev, 20, null, 70, 70, self_dev, 3, 0, out_dev, None),
        lib.silo_gpu_distance_cross(1, rows_dev, 20, columns_dev, 70, 70, self_dev, 3, 0, null, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_distance_cross" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_distance_cross(0, rows_dev, 0, columns_dev, 70, 70, self_dev, 3, 0, out_dev, None) == 0
    assert lib.silo_gpu_distance_cross(0, rows_dev, 20, columns_dev, 0, 70, self_dev, 3, 0, out_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (read() == SENTINEL).all()
    # no positions: every pair has (0, 0)
    zeros = np.zeros((20, 70), dtype=np.uint32)
    for min_compared in (0, 1):
        binding._check(lib.silo_gpu_memset_async(out_dev, FILL, (words + GUARD) * 4, None))
        binding._check(lib.silo_gpu_distance_cross(0, rows_dev, 20, columns_dev, 70, 0, self_dev, 0, min_compared, out_dev, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        got = read()
        assert np.array_equal(got[:words].reshape(20, 70, 2), cells_of(zeros, zeros, self_columns, 0, min_compared)) and (got[words:] == SENTINEL).all()
    # the valid call on the same buffers
    binding._check(lib.silo_gpu_memset_async(out_dev, FILL, (words + GUARD) * 4, None))
    binding._check(lib.silo_gpu_distance_cross(0, rows_dev, 20, columns_dev, 70, 70, self_dev, 3, 0, out_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    got = read()
    assert np.array_equal(got[:words].reshape(20, 70, 2), cells_of(*cross_counts(chars[:20], chars[20:], NUC_VALID), self_columns, 3, 0))
    assert (got[words:] == SENTINEL).all()
    for pointer in (rows_dev, columns_dev, self_dev, out_dev):
        binding.device_free(pointer)
