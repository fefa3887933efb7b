"""The weights kernel of MinimumSpanningTree (K13, csrc/silo_gpu_distance.hip) through silo_gpu_distance_weights, against the
numpy reference of tests/spanning_reference.py (pinned without a GPU by tests/test_spanning_reference.py).

tests/test_minimum_spanning_tree_gpu.py reaches it through JSON and the engine.  Here the entry gets the shapes where the kernel
takes another path — the same as tests/test_distance_within_gpu.py gives the kernel it shares its walk with: rows around the
16 x 64 tile, around a 64 x 64 block of the matrix and past the 2 048 rows one pack call takes; positions around a word and around
the chunk of words a block stages; both bounds at, below and above values that occur; tiles that stop early, tiles that must not,
and an edge tile; special rows; the refusals.  Every case has the output filled with 0xA5 bytes before the launch and four guard
words behind it, and is checked for symmetry, a diagonal of UINT32_MAX, equality with the reference, and against
silo_gpu_distance_within on the same planes: the bit matrix is `weights != UINT32_MAX`.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.clusters_reference import adjacency_words, pair_counts, unpack_bits  # noqa: E402
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402
from tests.spanning_reference import NO_EDGE, weights_of  # noqa: E402

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}
TR = 16   # SILO_GPU_WITHIN_TILE_ROWS: what the row counts below stand around ...
TC = 64   # SILO_GPU_WITHIN_TILE_COLS: ... with this
C = 16    # SILO_GPU_WITHIN_CHUNK_WORDS: what the positions below stand around
FILL = 0xA5
SENTINEL = 0xA5A5A5A5
GUARD = 4
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
LONG = 4103            # positions of the early-exit cases: several chunks
NO_BOUND = NO_EDGE


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.WITHIN_TILE_ROWS, binding.WITHIN_TILE_COLS, binding.WITHIN_CHUNK_WORDS, binding.MAX_SPANNING_ROWS) == (TR, TC, C, 8192)
    assert LONG > 2 * 64 * C and binding.NO_EDGE == NO_EDGE


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

    def check(self, max_distance, min_compared, within=True):
        """The matrix uint32 [n][n] after the checks."""
        from silo_amd import binding

        n = self.n
        out = binding.distance_weights(self.name, self.planes, n, self.positions, max_distance, min_compared, fill=FILL, guard_words=GUARD)
        assert len(out) == n * n + GUARD and (out[n * n:] == SENTINEL).all(), "the guard words were written"
        got = out[:n * n].reshape(n, n)
        assert np.array_equal(got, got.T), "not symmetric"
        assert (got.diagonal() == NO_EDGE).all(), "the diagonal"
        want = weights_of(self.differing, self.compared, max_distance, min_compared)
        assert np.array_equal(got, want), (self.name, n, self.positions, max_distance, min_compared, np.argwhere(got != want)[:5])
        if within:  # the kernel that shares the walk
            bits = binding.distance_within(self.name, self.planes, n, self.positions, max_distance, min_compared, fill=FILL)
            assert np.array_equal(unpack_bits(bits.reshape(n, adjacency_words(n)), n), got != NO_EDGE)
        return got


def _occurring(packed):
    """(d, c): a distance and a compared count that occur among the pairs, in the middle of what occurs."""
    upper = np.triu_indices(packed.n, 1)
    distances, counts = np.sort(packed.differing[upper]), np.sort(packed.compared[upper])
    return int(distances[len(distances) // 2]), int(counts[len(counts) // 2])


# ---- a: rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("n", [1, 2, TR - 1, TR, TR + 1, TC - 1, TC, TC + 1, TC + TR - 1, TC + TR + 1, 2 * TC + 1, 3 * TC + TR + 3])
def test_rows_around_the_tile_and_a_block(built, name, n):
    assert (1, 2, 15, 16, 17, 63, 64, 65, 79, 81, 129, 211) == (1, 2, TR - 1, TR, TR + 1, TC - 1, TC, TC + 1, TC + TR - 1, TC + TR + 1, 2 * TC + 1, 3 * TC + TR + 3)
    rng = np.random.default_rng(3100 + n)
    with Packed(name, _draw(rng, name, n, 130, changed=0.05)) as packed:
        if n == 1:
            assert packed.check(NO_BOUND, 0).tolist() == [[NO_EDGE]]
            return
        d, c = _occurring(packed)
        some = packed.check(d, 0)
        everything = packed.check(NO_BOUND, 0)
        assert (everything != NO_EDGE).sum() == n * (n - 1) and (some != NO_EDGE).any()
        packed.check(d, c)
        if n > 2 * TR:
            assert (some != NO_EDGE).sum() < n * (n - 1) and len(np.unique(some)) > 3


# ---- b: positions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("positions", [1, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1, LONG])
def test_positions_around_a_word_and_a_chunk(built, name, positions):
    assert (1023, 1024, 1025, 4103) == (64 * C - 1, 64 * C, 64 * C + 1, LONG)
    rng = np.random.default_rng(3200 + positions)
    with Packed(name, _draw(rng, name, 80, positions, changed=0.02 if positions > 100 else 0.3)) as packed:
        d, c = _occurring(packed)
        some = packed.check(d, c)
        assert (packed.check(NO_BOUND, 0) != NO_EDGE).sum() == 80 * 79
        packed.check(0, 0)
        if positions > 1:
            assert 0 < (some != NO_EDGE).sum() < 80 * 79


# ---- c: the two bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_bounds_at_below_and_above_values_that_occur(built, name):
    rng = np.random.default_rng(3300)
    with Packed(name, _draw(rng, name, 80, 130, changed=0.08)) as packed:
        d, c = _occurring(packed)
        assert d >= 1 and c >= 1
        edges = {}
        for max_distance in (0, d - 1, d, NO_BOUND):
            for min_compared in (0, c, c + 1, NO_BOUND):
                edges[max_distance, min_compared] = int((packed.check(max_distance, min_compared) != NO_EDGE).sum())
        assert edges[d - 1, 0] < edges[d, 0] < edges[NO_BOUND, 0] == 80 * 79   # a pair at exactly d
        assert edges[NO_BOUND, c + 1] < edges[NO_BOUND, c] < edges[NO_BOUND, 0]  # a pair at exactly c
        assert all(count == 0 for (_, min_compared), count in edges.items() if min_compared == NO_BOUND)


# ---- d: early exit -----------------------------------------------------------------------------------------------------------------
def _prefix(name, shift):
    """64 valid symbols, symbol (position + shift) of the valid ones in a circle: two such prefixes differ at every position unless
    their shifts are equal modulo the number of valid symbols."""
    valid = np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8)
    return valid[(np.arange(64) + shift) % len(valid)]


@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("with_the_pair", [True, False])
def test_a_tile_of_far_pairs_stops_unless_one_pair_is_near(built, name, with_the_pair):
    """Rows 0 .. 15 against rows 64 .. 127 is one tile; the two groups differ at every one of the first 64 positions.  With rows 3
    and 74 made equal but for one position of the last word, the tile must walk to the end for that pair; without, it stops after
    its first chunk and its cells — and those of its transpose — are UINT32_MAX (not the 0xA5 bytes the output held)."""
    rng = np.random.default_rng(3500)
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
            assert (packed.check(0, 0)[:TR, TC:] == NO_EDGE).all()
            got = packed.check(5, 0)
            assert got[3, 74] == 1 and got[74, 3] == 1 and (got[:TR, TC:] != NO_EDGE).sum() == 1 and (got[TC:, :TR] != NO_EDGE).sum() == 1
        else:
            assert across.min() >= 64
            got = packed.check(5, 0)
            assert (got[:TR, TC:] == NO_EDGE).all() and (got[TC:, :TR] == NO_EDGE).all() and (got[:TR, :TR] != NO_EDGE).any()
        assert (packed.check(NO_BOUND, 0) != NO_EDGE).sum() == (packed.check(LONG, 0) != NO_EDGE).sum() == 2 * TC * (2 * TC - 1)  # nothing stops


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_an_edge_tile_whose_rows_past_n_would_have_distance_zero(built, name):
    """n = 69: the tile of rows 64 .. 79 against columns 64 .. 127 holds 5 x 5 pairs of rows that exist — which differ at every
    one of the first 64 positions — and rows past n, staged as zeros, whose distance to anything is 0: they must neither become
    edges, nor be written, nor keep the answer from being exact."""
    rng = np.random.default_rng(3600)
    n = TC + 5
    chars = _draw(rng, name, n, LONG, changed=0.0)
    for row in range(n):
        chars[row, :64] = _prefix(name, row % 5)
    with Packed(name, chars) as packed:
        assert packed.differing[TC:, TC:][~np.eye(5, dtype=bool)].min() >= 64
        got = packed.check(5, 0)
        assert (got[TC:, TC:] == NO_EDGE).all() and (got[:TC, :TC] != NO_EDGE).any()
        packed.check(0, 0)
        packed.check(64, 0)


# ---- e: special rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_special_rows(built, name):
    """Identical rows are an edge of weight 0; a row of the missing symbol has (0, 0) against everything, an edge of weight 0 to
    every row with min_compared 0 and to none with 1; the bytes a, ? and NUL are not valid."""
    all_chars, valid_chars = ALPHABETS[name]
    positions = 150
    rng = np.random.default_rng(3700)
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
        assert at_zero[0, 1] == 0 and at_zero[3, 5] == 0 and at_zero[3, 4] == NO_EDGE and at_zero[4, 5] == NO_EDGE
        assert (at_zero[2] == 0).sum() == 6 and (at_zero[6] == 0).sum() == 6 and at_zero[2, 6] == 0
        at_one = packed.check(0, 1)
        assert (at_one[2] == NO_EDGE).all() and (at_one[6] == NO_EDGE).all() and at_one[0, 1] == 0 and at_one[3, 5] == 0
        assert packed.compared[3, 5] == positions - 3
        assert packed.check(0, positions - 3)[3, 5] == 0 and packed.check(0, positions - 2)[3, 5] == NO_EDGE
        assert packed.check(positions - 3, 0)[4, 5] == positions - 3 and packed.check(positions - 4, 0)[4, 5] == NO_EDGE
        unbounded = packed.check(NO_BOUND, 0)
        assert unbounded[3, 4] == positions and unbounded[2, 3] == 0


# ---- f: past the rows of one pack call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("nuc", 2049), ("aa", 2049), ("nuc", 4097)])
def test_more_rows_than_one_pack_call_takes(built, name, n):
    rng = np.random.default_rng(3800 + n)
    group = rng.integers(0, 40, size=n)
    chars = rng.choice(np.frombuffer(ALPHABETS[name][1].encode(), dtype=np.uint8), size=(40, 70))[group]   # 40 kinds of row, far apart ...
    redrawn = rng.random(chars.shape) < 0.01                # ... and near copies of them
    chars[redrawn] = rng.choice(np.frombuffer(ALPHABETS[name][0].encode(), dtype=np.uint8), size=int(redrawn.sum()))
    with Packed(name, chars) as packed:
        got = packed.check(1, 60) != NO_EDGE
        assert 0 < got.sum() < n * (n - 1) // 10 and got[:, 2048:].any() and got[2048:, :64].any()


# ---- g: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_no_rows_and_no_positions(built):
    """8 193 rows, an alphabet that does not exist, NULL buffers: SILO_GPU_ERR_INVALID_ARGUMENT and nothing written; no rows:
    success and nothing written; no positions: the matrix of "compared = distance = 0"; the next valid call answers exactly."""
    from silo_amd import binding

    lib = binding.load_library()
    rng = np.random.default_rng(3900)
    chars = _draw(rng, "nuc", 70, 70)
    planes_dev = binding.distance_pack_rows("nuc", chars)
    cells = 70 * 70
    out_dev = binding.device_malloc((cells + GUARD) * 4, fill=FILL)
    null = ctypes.c_void_p(0)

    def read():
        return binding.device_read(out_dev, np.uint32, cells + GUARD)

    refused = [
        lib.silo_gpu_distance_weights(0, planes_dev, binding.MAX_SPANNING_ROWS + 1, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_weights(2, planes_dev, 70, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_weights(-1, planes_dev, 70, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_weights(0, null, 70, 70, 3, 0, out_dev, None),
        lib.silo_gpu_distance_weights(1, planes_dev, 70, 70, 3, 0, null, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_distance_weights" in lib.silo_gpu_last_error()
    assert lib.silo_gpu_distance_weights(0, planes_dev, 0, 70, 3, 0, out_dev, None) == 0
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert (read() == SENTINEL).all()
    # no positions: every pair has (0, 0)
    star = np.zeros((70, 70), dtype=np.uint32)
    np.fill_diagonal(star, NO_EDGE)
    for min_compared, want in ((0, star), (1, np.full((70, 70), NO_EDGE, dtype=np.uint32))):
        binding._check(lib.silo_gpu_memset_async(out_dev, FILL, (cells + GUARD) * 4, None))
        binding._check(lib.silo_gpu_distance_weights(0, planes_dev, 70, 0, 0, min_compared, out_dev, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        got = read()
        assert np.array_equal(got[:cells].reshape(70, 70), want) and (got[cells:] == SENTINEL).all()
    # the valid call on the same buffers
    binding._check(lib.silo_gpu_distance_weights(0, planes_dev, 70, 70, 3, 0, out_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    got = read()
    assert np.array_equal(got[:cells].reshape(70, 70), weights_of(*pair_counts(chars, NUC_VALID), 3, 0))
    assert (got[cells:] == SENTINEL).all()
    for pointer in (planes_dev, out_dev):
        binding.device_free(pointer)
