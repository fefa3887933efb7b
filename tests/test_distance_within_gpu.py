"""The bit-per-pair kernel of Clusters (K12, csrc/silo_gpu_distance.hip) through silo_gpu_distance_within, against the numpy
reference of tests/clusters_reference.py (pinned without a GPU by tests/test_clusters_reference.py).

tests/test_clusters_gpu.py reaches it through JSON and the engine.  Here the entry gets the shapes where its kernels take another
path: rows around the 16 x 64 tile, around a word of the matrix and past the 2 048 rows one pack call takes; positions around a
word and around the chunk of words a block stages; both bounds at, below and above values that occur; tiles that stop early, tiles
that must not, and an edge tile; special rows; the refusals.  Every case has the output filled with 0xA5 bytes before the launch
and four guard words behind it, and is checked for symmetry, a clear diagonal, zero bits at or past n and equality with the
reference.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.clusters_reference import NO_BOUND, adjacency_words, linked_pairs, pack_bits, pair_counts, unpack_bits  # noqa: E402
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}
TR = 16   # SILO_GPU_WITHIN_TILE_ROWS: what the row counts below stand around ...
TC = 64   # SILO_GPU_WITHIN_TILE_COLS: ... with this
C = 16    # SILO_GPU_WITHIN_CHUNK_WORDS: what the positions below stand around
FILL = 0xA5
SENTINEL = 0xA5A5A5A5A5A5A5A5
GUARD = 4
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
LONG = 4103            # positions of the early-exit cases: several chunks at any chunk size up to 32 words


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.WITHIN_TILE_ROWS, binding.WITHIN_TILE_COLS, binding.WITHIN_CHUNK_WORDS, binding.MAX_CLUSTER_ROWS) == (TR, TC, C, 8192)
    assert LONG > 2 * 64 * C


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
    """The planes of chars on the device, and the reference's two counts per pair: several bounds are asked of one packing."""

    def __init__(self, name, chars):
        from silo_amd import binding

        self.name, self.chars = name, chars
        self.n, self.positions = chars.shape
        self.planes = binding.distance_pack_rows(name, chars, fill=FILL)
        self.differing, self.compared = pair_counts(chars, ALPHABETS[name][1])

    def __enter__(self):
        return self

    def __exit__(self, *_):
        from silo_amd import binding

        binding.device_free(self.planes)

    def check(self, max_distance, min_compared):
        """The matrix as bool [n][n] after the four checks."""
        from silo_amd import binding

        n, aw = self.n, adjacency_words(self.n)
        out = binding.distance_within(self.name, self.planes, n, self.positions, max_distance, min_compared, fill=FILL, guard_words=GUARD)
        assert len(out) == n * aw + GUARD and (out[n * aw:] == SENTINEL).all(), "the guard words were written"
        words = out[:n * aw].reshape(n, aw)
        bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little").astype(bool)
        assert not bits[:, n:].any(), "bits at or past n"
        got = bits[:, :n]
        assert np.array_equal(got, got.T), "not symmetric"
        assert not got.diagonal().any(), "the diagonal"
        want = linked_pairs(self.differing, self.compared, max_distance, min_compared)
        assert np.array_equal(got, want), (self.name, n, self.positions, max_distance, min_compared)
        assert np.array_equal(words, pack_bits(want))
        return got


def _occurring(packed):
    """(d, c): a distance and a compared count that occur among the pairs, in the middle of what occurs."""
    upper = np.triu_indices(packed.n, 1)
    distances, counts = np.sort(packed.differing[upper]), np.sort(packed.compared[upper])
    return int(distances[len(distances) // 2]), int(counts[len(counts) // 2])


# ---- a: rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("n", [1, 2, TR - 1, TR, TR + 1, 2 * TR + 1, TC - 1, TC, TC + 1, TC + TR - 1, TC + TR + 1, 2 * TC - 1, 2 * TC, 2 * TC + 1, 3 * TC + TR + 3])
def test_rows_around_the_tile_and_a_word(built, name, n):
    assert {1, 2, 15, 16, 17, 63, 64, 65, 129} <= {1, 2, TR - 1, TR, TR + 1, TC - 1, TC, TC + 1, 2 * TC + 1}
    rng = np.random.default_rng(2100 + n)
    with Packed(name, _draw(rng, name, n, 130, changed=0.05)) as packed:
        if n == 1:
            assert not packed.check(NO_BOUND, 0).any()
            return
        d, c = _occurring(packed)
        some = packed.check(d, 0)
        everything = packed.check(NO_BOUND, 0)
        assert everything.sum() == n * (n - 1) and some.any()
        packed.check(d, c)
        if n > 2 * TR:
            assert some.sum() < everything.sum()


# ---- b: positions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("positions", [1, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1, LONG])
def test_positions_around_a_word_and_a_chunk(built, name, positions):
    assert {1023, 1025} <= {64 * C - 1, 64 * C + 1}
    rng = np.random.default_rng(2200 + positions)
    with Packed(name, _draw(rng, name, 80, positions, changed=0.02 if positions > 100 else 0.3)) as packed:
        d, c = _occurring(packed)
        some = packed.check(d, c)
        assert packed.check(NO_BOUND, 0).sum() == 80 * 79
        packed.check(0, 0)
        if positions > 1:
            assert 0 < some.sum() < 80 * 79


# ---- c: the two bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_bounds_at_below_and_above_values_that_occur(built, name):
    rng = np.random.default_rng(2300)
    with Packed(name, _draw(rng, name, 80, 130, changed=0.08)) as packed:
        d, c = _occurring(packed)
        assert d >= 1 and c >= 1
        linked = {}
        for max_distance in (0, d - 1, d, NO_BOUND):
            for min_compared in (0, c, c + 1, NO_BOUND):
                linked[max_distance, min_compared] = int(packed.check(max_distance, min_compared).sum())
        assert linked[d - 1, 0] < linked[d, 0] < linked[NO_BOUND, 0] == 80 * 79   # a pair at exactly d
        assert linked[NO_BOUND, c + 1] < linked[NO_BOUND, c] < linked[NO_BOUND, 0]  # a pair at exactly c
        assert all(count == 0 for (_, min_compared), count in linked.items() if min_compared == NO_BOUND)


# ---- d: early exit -----------------------------------------------------------------------------------------------------------------
def _prefix(name, shift):
    """64 valid symbols, symbol (position + shift) of the valid ones in a circle: two such prefixes differ at every position unless
    their shifts are equal modulo the number of valid symbols."""
    valid = np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8)
    return valid[(np.arange(64) + shift) % len(valid)]


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_a_pair_whose_differences_all_lie_in_the_last_word(built, name):
    rng = np.random.default_rng(2400)
    chars = _draw(rng, name, 80, LONG, changed=0.02)
    valid = np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8)
    chars[70] = chars[3] = valid[np.arange(LONG) % len(valid)]
    chars[70, [4096, 4100, 4102]] = valid[(np.array([4096, 4100, 4102]) + 1) % len(valid)]
    with Packed(name, chars) as packed:
        assert packed.differing[3, 70] == 3 and packed.compared[3, 70] == LONG
        assert not packed.check(2, 0)[3, 70]
        assert packed.check(3, 0)[3, 70]
        assert packed.check(3, LONG)[3, 70] and not packed.check(3, LONG + 1).any()


@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("with_the_pair", [True, False])
def test_a_tile_of_far_pairs_stops_unless_one_pair_is_near(built, name, with_the_pair):
    """Rows 0 .. 15 against rows 64 .. 127 is one tile; the two groups differ at every one of the first 64 positions.  With rows 3
    and 74 made equal but for one position of the last word, the tile must walk to the end for that pair; without, it stops after
    its first chunk and its words are zeros (not the 0xA5 bytes the output held)."""
    rng = np.random.default_rng(2500)
    chars = _draw(rng, name, 2 * TC, LONG, changed=0.0)
    chars[:TC, :64] = _prefix(name, 0)
    chars[TC:, :64] = _prefix(name, 1)
    tail = rng.random((2 * TC, LONG - 64)) < 0.0003   # a few differences behind the prefix, within the groups too
    chars[:, 64:][tail] = ord("-")
    if with_the_pair:
        chars[3, :64] = chars[74, :64] = _prefix(name, 2)
        chars[74, 64:] = chars[3, 64:]
        chars[74, LONG - 1] = ord("A") if chars[3, LONG - 1] != ord("A") else ord("C")
    with Packed(name, chars) as packed:
        across = packed.differing[:TR, TC:]
        if with_the_pair:
            assert across[3, 10] == 1 and np.sort(across.ravel())[1] >= 64
            assert not packed.check(0, 0)[:TR, TC:].any()
            tile = packed.check(5, 0)[:TR, TC:]
            assert tile[3, 10] and tile.sum() == 1
        else:
            assert across.min() >= 64
            got = packed.check(5, 0)
            assert not got[:TR, TC:].any() and got[:TR, :TR].any()
        assert packed.check(NO_BOUND, 0).sum() == packed.check(LONG, 0).sum() == 2 * TC * (2 * TC - 1)  # nothing stops, all but the diagonal


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_an_edge_tile_whose_rows_past_n_would_have_distance_zero(built, name):
    """n = 69: the tile of rows 64 .. 79 against columns 64 .. 127 holds 5 x 5 pairs of rows that exist — which differ at every
    one of the first 64 positions — and rows past n, staged as zeros, whose distance to anything is 0: they must neither be linked
    nor keep the answer from being exact."""
    rng = np.random.default_rng(2600)
    n = TC + 5
    chars = _draw(rng, name, n, LONG, changed=0.0)
    for row in range(n):
        chars[row, :64] = _prefix(name, row % 5)
    with Packed(name, chars) as packed:
        assert packed.differing[TC:, TC:][~np.eye(5, dtype=bool)].min() >= 64
        got = packed.check(5, 0)
        assert not got[TC:, TC:].any() and got[:TC, :TC].any()
        packed.check(0, 0)
        packed.check(64, 0)


# ---- e: special rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_special_rows(built, name):
    """Identical rows are linked at 0; a row of the missing symbol has (0, 0) against everything, itself a link to every row with
    min_compared 0 and to none with 1; the bytes a, ? and NUL are not valid."""
    all_chars, valid_chars = ALPHABETS[name]
    positions = 150
    rng = np.random.default_rng(2700)
    ordinary = _draw(rng, name, 1, positions, changed=0.3)[0]
    valid = np.frombuffer(valid_chars.encode(), dtype=np.uint8)
    everywhere = valid[np.arange(positions) % len(valid)]
    shifted = valid[(np.arange(positions) + 1) % len(valid)]
    strange = everywhere.copy()
    strange[[0, 64, 149]] = [ord("a"), ord("?"), 0]
    missing = np.full(positions, ord(all_chars[-1]), dtype=np.uint8)
    chars = np.stack([ordinary, ordinary, missing, everywhere, shifted, strange, missing])
    with Packed(name, chars) as packed:
        at_zero = packed.check(0, 0)
        assert at_zero[0, 1] and at_zero[3, 5] and not at_zero[3, 4] and not at_zero[4, 5]
        assert at_zero[2].sum() == 6 and at_zero[6].sum() == 6 and at_zero[2, 6]
        at_one = packed.check(0, 1)
        assert not at_one[2].any() and not at_one[6].any() and at_one[0, 1] and at_one[3, 5]
        assert packed.compared[3, 5] == positions - 3
        assert packed.check(0, positions - 3)[3, 5] and not packed.check(0, positions - 2)[3, 5]
        assert packed.check(positions - 3, 0)[4, 5] and not packed.check(positions - 4, 0)[4, 5]


# ---- f: past the rows of one pack call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("nuc", 2049), ("aa", 2049), ("nuc", 4097)])
def test_more_rows_than_one_pack_call_takes(built, name, n):
    rng = np.random.default_rng(2800 + n)
    group = rng.integers(0, 40, size=n)
    chars = rng.choice(np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8), size=(40, 70))[group]   # 40 kinds of row, far apart ...
    redrawn = rng.random(chars.shape) < 0.01                # ... and near copies of them
    chars[redrawn] = rng.choice(np.frombuffer(ALPHABETS[name][0].encode(), dtype=np.uint8), size=int(redrawn.sum()))
    with Packed(name, chars) as packed:
        got = packed.check(1, 60)
        assert 0 < got.sum() < n * (n - 1) // 10 and got[:, 2048:].any() and got[2048:, :64].any()


# ---- g: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_no_rows_and_no_positions(built):
    """8 193 rows, an alphabet that does not exist, NULL buffers: SILO_GPU_ERR_INVALID_ARGUMENT and nothing written; no rows:
    success and nothing written; no positions: the matrix of "compared = distance = 0"; the next valid call answers exactly."""
    from silo_amd import binding

    lib = binding.load_library()
    rng = np.random.default_rng(2900)
    chars = _draw(rng, "nuc", 70, 70)
    planes_dev = binding.distance_pack_rows("nuc", chars)
    words = 70 * 2
    out_dev = binding.device_malloc((words + GUARD) * 8, fill=FILL)
    null = ctypes.c_void_p(0)

    def read():
        return binding.device_read(out_dev, np.uint64, words + GUARD)

    refused = [
        lib.silo_gpu_distance_within(0, planes_dev, binding.MAX_CLUSTER_ROWS + 1, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_within(2, planes_dev, 70, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_within(-1, planes_dev, 70, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_within(0, null, 70, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_within(1, planes_dev, 70, 70, 3, 0, null, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_distance_within" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_distance_within(0, planes_dev, 0, 70, 3, 0, out_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (read() == SENTINEL).all()
    # the old limit is not this entry's, and stays the pack entry's
    assert lib.silo_gpu_distance_pack(0, planes_dev, binding.MAX_DISTANCE_ROWS + 1, 70, out_dev, None) == INVALID_ARGUMENT
    # no positions: every pair has (0, 0)
    for min_compared, want in ((0, ~np.eye(70, dtype=bool)), (1, np.zeros((70, 70), dtype=bool))):
        binding._check(lib.silo_gpu_memset_async(out_dev, FILL, (words + GUARD) * 8, None))
        binding._check(lib.silo_gpu_distance_within(0, planes_dev, 70, 0, 0, min_compared, out_dev, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        got = read()
        assert np.array_equal(unpack_bits(got[:words], 70), want) and np.array_equal(got[:words].reshape(70, 2), pack_bits(want))
        assert (got[words:] == SENTINEL).all()
    # the valid call on the same buffers
    binding._check(lib.silo_gpu_distance_within(0, planes_dev, 70, 70, 3, 0, out_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    got = read()
    assert np.array_equal(got[:words].reshape(70, 2), pack_bits(linked_pairs(*pair_counts(chars, NUC_VALID), 3, 0)))
    assert (got[words:] == SENTINEL).all()
    for pointer in (planes_dev, out_dev):
        binding.device_free(pointer)
