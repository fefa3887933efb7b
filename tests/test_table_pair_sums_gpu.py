"""The pairwise sums of count tables (K24, csrc/silo_gpu_pair_sums.hip) through silo_gpu_table_pair_sums, on numpy count tables
against tests/mean_distances_reference.py (pinned against a plain loop, against the sums of pair distances over rows and against a
loop over characters without a GPU by tests/test_mean_distances_reference.py).

Every comparison is an equality of all the output's bytes.  The output is filled with 0xA5 bytes before the launch and has 16 guard
bytes behind it, which must still hold 0xA5 afterwards.  Position counts stand around the 16 positions a block stages at a time and
around the 128 positions of a block's chunk; 4 103 gives 33 chunks.  1, 2 and 3 tables leave most of a tile of 16 x 16 pairs idle, 16
fill one tile, 17 need three and 64 all ten.  Every call carries several ranges — the whole table, its first and its last position
alone, two that overlap, one across a chunk's edge — out of order, so the jobs of many ranges are one grid.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.consensus_reference import VALID  # noqa: E402
from tests.mean_distances_reference import CHUNK, MASK64, MAX_RANGES, MAX_TABLES, POSITION_TILE, TILE, WORDS, pack, pair_index, pair_sums  # noqa: E402
from tests.test_mutations_comparison_reference import _skewed  # noqa: E402

FILL = 0xA5
SENTINEL = 0xA5A5A5A5A5A5A5A5
GUARD = 16
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT
POSITIONS = [1, POSITION_TILE - 1, POSITION_TILE, POSITION_TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 4103]
TABLES = [1, 2, 3, TILE, TILE + 1, MAX_TABLES]
NEAR = 2**32 - 1  # the highest coverage


def _ranges(positions):
    ranges = [(positions - 1, positions), (0, positions), (0, 1)]
    if positions >= 4:
        ranges += [(positions // 2, positions), (positions // 4, 3 * positions // 4 + 1)]  # they overlap
    if positions >= CHUNK + 5:
        ranges.insert(1, (CHUNK - 3, CHUNK + 5))  # across a chunk's edge of the whole table, a chunk of its own
    return ranges


def _check(alphabet, counts, ranges, calls=1):
    """The sums as the device leaves them, after the comparison of every byte with the reference."""
    from silo_amd import binding

    want = pair_sums(counts, ranges)
    out, status = binding.table_pair_sums(alphabet, counts, ranges, fill=FILL, guard_bytes=GUARD, calls=calls)
    case = (alphabet, counts.shape, ranges[:6], calls)
    assert status == 0, case
    tables = counts.shape[0]
    assert len(out) == len(ranges) * (tables * (tables + 1) // 2) * WORDS + GUARD // 8
    assert (out[-GUARD // 8:] == SENTINEL).all(), "the guard bytes were written"
    words = pack(want)
    assert np.array_equal(out[:-GUARD // 8], words), (case, np.argwhere(out[:-GUARD // 8] != words)[:5])
    return want


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.PAIR_SUM_POSITION_TILE, binding.PAIR_SUM_CHUNK, binding.PAIR_SUM_TILE) == (POSITION_TILE, CHUNK, TILE) == (16, 128, 16)
    assert (binding.MAX_PAIR_SUM_TABLES, binding.MAX_PAIR_SUM_RANGES, binding.PAIR_SUM_WORDS) == (MAX_TABLES, MAX_RANGES, WORDS) == (64, 256, 5)
    for edge in (binding.PAIR_SUM_POSITION_TILE, binding.PAIR_SUM_CHUNK):
        assert {edge - 1, edge, edge + 1} <= set(POSITIONS)
    assert {1, 4103} <= set(POSITIONS) and set(TABLES) == {1, 2, 3, binding.PAIR_SUM_TILE, binding.PAIR_SUM_TILE + 1, binding.MAX_PAIR_SUM_TABLES}


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("positions", POSITIONS)
def test_shapes(built, alphabet, tables, positions):
    rng = np.random.default_rng(24000 + 100 * positions + tables + (alphabet == "aa"))
    counts = _skewed(rng, alphabet, tables, positions)
    ranges = _ranges(positions)
    want = _check(alphabet, counts, ranges)
    if positions >= 4000:
        whole = want[ranges.index((0, positions))]
        assert all(int(whole[pair_index(g, g, tables)][2]) > 0 for g in range(tables))  # segregating sites in every table
        assert int(whole[:, 0].sum()) > 0 and (tables == 1 or int(whole[pair_index(0, tables - 1, tables)][2]) > 0)  # and fixed differences


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_256_single_positions(built, alphabet):
    rng = np.random.default_rng(24100 + (alphabet == "aa"))
    counts = _skewed(rng, alphabet, 3, 300)
    starts = rng.permutation(300)[:MAX_RANGES]
    _check(alphabet, counts, [(int(p), int(p) + 1) for p in starts])


def _heavy(alphabet, positions, places):
    """Two tables whose coverage is the highest a coverage can be at `places`, in symbols the other table does not hold there, and
    small elsewhere."""
    rng = np.random.default_rng(24200 + positions)
    counts = rng.integers(0, 3, size=(2, positions, len(VALID[alphabet]))).astype(np.uint32)
    for place in places:
        counts[:, place] = 0
        counts[0, place, 1] = NEAR - 5
        counts[0, place, 2] = 5
        counts[1, place, 3] = NEAR - 1
        counts[1, place, 4] = 1
    return counts


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_the_high_words(built, alphabet):
    """Three positions with coverages next to 2^32 in both tables: each adds about 2^64 to the pair's sums.  In one position tile a
    thread carries into its own high word; in two chunks the blocks' adds on the low word wrap and carry across blocks."""
    for positions, places in ((40, (3, 4, 20)), (300, (5, CHUNK + 2, CHUNK + 12)), (3 * CHUNK, (CHUNK - 1, CHUNK, 2 * CHUNK))):
        counts = _heavy(alphabet, positions, places)
        want = _check(alphabet, counts, [(0, positions), (places[0], places[0] + 1)])
        differences, compared, sites = (int(v) for v in want[0][pair_index(0, 1, 2)])
        assert differences >> 64 >= 2 and compared >> 64 >= 2 and sites >= 3  # diff_hi and cmp_hi are not 0
        assert int(want[0][pair_index(0, 0, 2)][1]) >> 64 >= 1 and int(want[0][pair_index(1, 1, 2)][0]) > 0
        assert int(want[1][pair_index(0, 1, 2)][1]) == NEAR * NEAR <= MASK64  # one position's term fits 64 bits


# (what it is about, the counts of one position in table 0 and in table 1 as "-ACGT", (differences, compared, sites) of (0, 0), (0, 1), (1, 1))
HAND_MADE = [
    ("coverage 0 in one table", [0, 0, 0, 0, 0], [0, 4, 1, 0, 0], (0, 0, 0), (0, 0, 0), (4, 10, 1)),
    ("coverage 1: no pair within", [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], (0, 0, 0), (1, 1, 1), (0, 0, 0)),
    ("one symbol only", [0, 7, 0, 0, 0], [0, 3, 0, 0, 0], (0, 21, 0), (0, 21, 0), (0, 3, 0)),
    ("two symbols", [0, 2, 3, 0, 0], [0, 1, 1, 0, 0], (6, 10, 1), (5, 10, 0), (1, 1, 1)),
    ("no shared symbol", [2, 0, 0, 0, 1], [0, 5, 0, 2, 0], (2, 3, 1), (21, 21, 1), (10, 21, 1)),
]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_hand_made_positions_at_the_ends_of_a_tile_and_of_a_chunk(built, alphabet):
    """Each hand-made position alone in a range, at the first and last position of a position tile, of a chunk and of the tables; its two
    tables are the first and the LAST of 18 (two tiles of pairs), under tables that are empty there."""
    tables, positions = TILE + 2, 2 * CHUNK + 7
    places = [0, POSITION_TILE - 1, POSITION_TILE, CHUNK - 1, CHUNK, positions - 1]
    background = _skewed(np.random.default_rng(24300), alphabet, tables, positions)
    for what, first, last, within_first, between, within_last in HAND_MADE:
        counts = background.copy()
        for place in places:
            counts[:, place] = 0
            counts[0, place, :5] = first
            counts[tables - 1, place, :5] = last
        want = _check(alphabet, counts, [(place, place + 1) for place in places] + [(0, positions)])
        for of_place in want[:len(places)]:
            got = [tuple(int(v) for v in of_place[pair_index(g, h, tables)]) for g, h in ((0, 0), (0, tables - 1), (tables - 1, tables - 1))]
            assert got == [within_first, between, within_last], what
            assert sum(int(v) for v in of_place.reshape(-1)) == sum(sum(sums) for sums in got), what  # the empty tables between them: zeros


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_a_second_call_gives_the_same_bytes(built, alphabet):
    rng = np.random.default_rng(24400)
    counts = _skewed(rng, alphabet, 5, 3 * CHUNK + 11)
    once = _check(alphabet, counts, _ranges(counts.shape[1]))
    twice = _check(alphabet, counts, _ranges(counts.shape[1]), calls=2)  # (compared with the reference again: the sums are not doubled)
    assert np.array_equal(pack(once), pack(twice)) and int(once[2][0][0]) > 0


def test_refusals_leave_the_fill(built):
    from silo_amd import binding

    rng = np.random.default_rng(24500)
    counts = _skewed(rng, "nuc", 2, 70)

    def refused(alphabet=0, table=counts, ranges=((0, 70),), **told):
        out, status = binding.table_pair_sums(alphabet, table, ranges, fill=FILL, guard_bytes=GUARD, **told)
        assert status == INVALID_ARGUMENT, (alphabet, table.shape, ranges[:3], told)
        assert len(out) > GUARD // 8 and (out == SENTINEL).all()

    for alphabet in (2, -1):
        refused(alphabet=alphabet)
    for name in ("counts", "ranges", "out"):
        refused(null=(name,))
    refused(n_tables=0)
    refused(table=np.zeros((MAX_TABLES + 1, 70, 5), dtype=np.uint32))
    refused(n_ranges=0)
    refused(ranges=[(p, p + 1) for p in range(MAX_RANGES + 1)], table=_skewed(rng, "nuc", 1, MAX_RANGES + 1))
    refused(n_positions=0)
    for ranges in ([(5, 5)], [(6, 5)], [(0, 71)], [(70, 71)], [(0, 70), (3, 3)], [(0, 70), (69, 72)], [(0, 2**32 - 1)]):
        refused(ranges=ranges)
    assert "table_pair_sums" in binding.load_library().silo_gpu_last_error().decode()
    _check("nuc", counts, [(69, 70), (0, 70)])  # and the same tables are accepted
