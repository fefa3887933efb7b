"""The grouped mutation-count kernels (K7, csrc/silo_gpu_grouped.hip) through silo_gpu_mutations_grouped, against the plain numpy
reference of oracle/dense.py (grouped_mutation_counts, row_groups; pinned without a GPU by tests/test_grouped_reference.py).

tests/test_mutations_over_time_gpu.py reaches K7 through JSON and the engine at one shape.  Here the entry point gets the shapes
where its kernels take another path: words of 64 rows with exactly 4 and exactly 5 ranges (WORD_SEGMENTS), more ranges than a
block has threads (the strided LDS loops), amino acids, a derived position listed in several blocks of 16 mutations, 4 096
derived positions in LDS, dates on the bounds of their ranges, filters with padding bits, a table that is accumulated into, and
the refusals of the entry itself.  Every comparison is an exact integer equality.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402
from tests.test_kernels_gpu import AA_CHARS, NUC_CHARS, make_store, settle_positions, skewed_symbols  # noqa: E402

NO_GROUP = dense.NO_GROUP
UNBOUNDED = 0xFFFFFFFF


def _alphabet(name):
    from silo_amd import alphabet as alphabets

    return alphabets.ALPHABETS[name]


def _upload_mask(store, mask):
    if mask is None:
        return None
    ptr = store.bitset_alloc()
    store.bitset_upload(ptr, dense.pack_bits(mask))
    return ptr


def _grouped(store, filter_ptr, dates_ptr, ranges, cells, **options):
    return store.mutations_grouped(0, filter_ptr, dates_ptr, ranges, [p for p, _ in cells], [s for _, s in cells], **options)


def _in_range(dates, low, high):
    wide = dates.astype(np.int64)
    return (wide != 0) & (wide >= low) & (wide <= high)


# ---- a: group assignment -----------------------------------------------------------------------------------------------------
ASSIGN_ROWS = [1, 63, 64, 65, 2047, 2049, 16_385]  # rows are padded to 2 048: a word, a 256-byte line, the 16 384 rows of a position block
UNREACHED = (3_000_000_000, 3_000_000_100)


def _short_ranges(rng, count):
    """`count` ranges of 1-3 days, some touching ([a, b], [b + 1, c]), some a day or two apart, in a shuffled request order."""
    ranges, day = [], 2000
    for _ in range(count):
        length = int(rng.integers(1, 4))
        ranges.append((day, day + length - 1))
        day += length + int(rng.integers(0, 3))
    return [ranges[k] for k in rng.permutation(count)]


def _assignment_range_sets(rng):
    return {
        "one": [(100, 200)],
        "touching": [(100, 150), (151, 300)],
        "zero-zero": [(0, 0), (1, 5)],
        "everything": [(0, UNBOUNDED)],
        "unbounded-ends": [(60, UNBOUNDED), (0, 50)],
        "257": _short_ranges(rng, 257),
        "1024": _short_ranges(rng, 1024),
        "unreached": [(100, 200), UNREACHED, (300, 300)],
    }


def _assignment_dates(rng, n, ranges):
    """0, 1, 0xFFFFFFFF, every bound of a range and its two neighbours, and random values; nothing inside UNREACHED."""
    bounds = np.array([b for r in ranges if r != UNREACHED for b in r], dtype=np.int64)
    pool = np.unique(np.clip(np.concatenate([[0, 1, UNBOUNDED], bounds - 1, bounds, bounds + 1]), 0, UNBOUNDED))
    finite = int(bounds[bounds != UNBOUNDED].max()) if (bounds != UNBOUNDED).any() else 0
    dates = rng.choice(pool, size=n)
    near = rng.random(n) < 0.3
    dates[near] = rng.integers(0, finite + 50, size=int(near.sum()))
    far = rng.random(n) < 0.05
    dates[far] = rng.integers(0, 1 << 32, size=int(far.sum()))
    dates[_in_range(dates, *UNREACHED)] = 1
    if n >= len(pool):  # every special value occurs
        dates[rng.choice(n, size=len(pool), replace=False)] = pool
    return dates.astype(np.uint32)


@pytest.mark.parametrize("n", ASSIGN_ROWS)
def test_group_assignment_matches_numpy(built, n):
    """k_assign_groups: the range id of every row (read back from the scratch) and |filter ∩ range| (the coverage of a position
    where every row has a valid symbol), for dates on and beside every bound, touching ranges, [0, 0], the unbounded encodings,
    257 and 1 024 ranges in shuffled order, a range no date reaches; without a filter, with an empty one, a random one and one
    whose padding bits are set."""
    rng = np.random.default_rng(400 + n)
    sym = rng.integers(1, 5, size=(n, 1)).astype(np.uint8)
    cells = [(0, 1), (0, 3)]
    with make_store(n, [dict(name="s", alphabet="nuc", reference=np.ones(1, dtype=np.uint8))]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        padded_rows = store.row_words * 64
        assert padded_rows % 2048 == 0 and padded_rows >= n
        random_mask = rng.random(n) < 0.5
        all_ones = store.bitset_alloc()
        store.bitset_upload(all_ones, np.full(store.row_words, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))  # padding bits set
        assert dense.unpack_bits(store.bitset_download(all_ones), padded_rows).all()
        filters = [(None, np.ones(n, bool)), (_upload_mask(store, np.zeros(n, bool)), np.zeros(n, bool)),
                   (_upload_mask(store, random_mask), random_mask), (all_ones, np.ones(n, bool))]
        for name, ranges in _assignment_range_sets(rng).items():
            dates = _assignment_dates(rng, n, ranges)
            if name == "unreached":
                assert not _in_range(dates, *UNREACHED).any()
            dates_dev = store.upload_column(dates)
            for index, (filter_ptr, mask) in enumerate(filters):
                table, groups = _grouped(store, filter_ptr, dates_dev, ranges, cells, return_groups=True)
                want_groups = dense.row_groups(mask, dates, ranges)
                assert groups.shape == (padded_rows,)
                assert np.array_equal(groups[:n], want_groups), (name, index)
                assert (groups[n:] == NO_GROUP).all(), (name, index)
                cardinality = np.bincount(want_groups[want_groups != NO_GROUP], minlength=len(ranges))
                assert np.array_equal(table[0, :, 1], cardinality) and np.array_equal(table[1, :, 1], cardinality), (name, index)
                assert np.array_equal(table, dense.grouped_mutation_counts(sym, mask, dates, ranges, cells, [0, 1, 2, 3, 4])), (name, index)
                if name == "unreached":
                    assert not table[:, 1].any()
                if name == "zero-zero":
                    assert not table[:, 0].any()  # [0, 0] holds the NULL date only: no row
            if n >= 2047 and name == "touching":  # (the last filter: every row) rows in both ranges and rows in none
                assert set(np.unique(want_groups).tolist()) == {0, 1, NO_GROUP}
            store.free(dates_dev)


# ---- b: counts in every layout -------------------------------------------------------------------------------------------------
N_ROWS = 70_001
POSITIONS = 24
SETTLED = list(range(3, 10)) + list(range(17, 23))  # one symbol has nearly every row: derived under knob 4 = 0
SECOND_FREQUENT = 20                                   # a settled position with a second frequent symbol (one one-hot row)
ALL_FREQUENT = 13                                      # every symbol frequent: code planes / identity
ABSENT_AT = 6                                          # a settled position that lacks one valid symbol altogether
LISTED_POSITIONS = [5, SECOND_FREQUENT, ALL_FREQUENT, 0, ABSENT_AT, POSITIONS - 1]  # 0 and 23: skewed (three frequent symbols)
N_RANGES = 40
LAYOUTS = [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)]  # (knob 4: one-hot mode, knob 8: < 0 keeps the plane of the missing symbol)
LAYOUT_IDS = ["derived", "one-hot", "code-planes", "identity", "missing-plane"]


@functools.lru_cache(maxsize=None)
def _matrix(alphabet):
    """The columns of test_adaptive_code_planes_give_the_same_tables, then runs of the missing symbol, rows that are missing
    throughout and scattered ambiguity codes."""
    table = _alphabet(alphabet)
    rng = np.random.default_rng(2100 + table.count)
    sym = skewed_symbols(rng, N_ROWS, POSITIONS, alphabet)
    sym[:, ALL_FREQUENT] = rng.integers(0, table.missing, size=N_ROWS)  # every symbol but the missing one (the last id): its cells here would be runs of one
    settle_positions(rng, sym, SETTLED, alphabet)
    settle_positions(rng, sym, [SECOND_FREQUENT], alphabet, second=0.02)
    valid = list(table.valid_mutation_symbols)
    counts = np.bincount(sym[:, ABSENT_AT], minlength=table.count)
    by_count = sorted(valid, key=lambda s: counts[s])
    sym[sym[:, ABSENT_AT] == by_count[0], ABSENT_AT] = by_count[-1]  # the rarest valid symbol gives its rows to the dominant one
    # (few enough runs that finalize keeps them as runs: a list longer than a quarter of the 24-position plane would stay a plane)
    for row in rng.choice(N_ROWS, size=N_ROWS // 50, replace=False):
        start = int(rng.integers(0, POSITIONS))
        sym[row, start:start + int(rng.integers(1, 12))] = table.missing
    sym[rng.choice(N_ROWS, size=150, replace=False), :] = table.missing
    ambiguity = [s for s in range(table.count) if s not in valid and s != table.missing]
    cells = rng.integers(0, N_ROWS * POSITIONS, size=N_ROWS // 10)
    sym.reshape(-1)[cells] = rng.choice(ambiguity, size=len(cells))
    sym.setflags(write=False)
    return sym


def _layout_store(alphabet, knob4, knob8):
    sym = _matrix(alphabet)
    chars = NUC_CHARS if alphabet == "nuc" else AA_CHARS
    store = make_store(N_ROWS, [dict(name="a", alphabet=alphabet, reference=sym[0].copy())])
    store.tune(4, knob4)
    store.tune(8, knob8)
    store.tune(9, -1)  # no charge per kind of launch: with it a store this short would never mix layouts
    try:
        store.append_sequences(0, 0, chars[sym])
        store.finalize()
    except Exception:
        store.close()
        raise
    finally:
        store.tune(4, 0)
        store.tune(8, 0)
        store.tune(9, 0)
    return store


def _assert_layout(store, alphabet, knob4, knob8):
    """The store has the layout the parametrisation aims at (the assertions of test_adaptive_code_planes_give_the_same_tables)."""
    table = _alphabet(alphabet)
    full_planes = 3 if alphabet == "nuc" else 5
    if knob4 == 0 and knob8 == 0:
        assert store.scan_rows(0, 3, 10) == 0 and store.scan_rows(0, 17, 23) == 1 and store.scan_rows(0, SECOND_FREQUENT, SECOND_FREQUENT + 1) == 1
        assert store.scan_rows(0, ALL_FREQUENT, ALL_FREQUENT + 1) > 1 and store.scan_rows(0, 12, 13) >= 1 and 3 <= store.scan_rows(0, 0, 3) <= 6
        assert 0 < store.scan_escapes(0) <= N_ROWS * POSITIONS // 200
        assert store.scan_runs(0) > 0 and store.plane(0, 0, table.missing) is None
    elif knob4 == 0:
        # the plane of the missing symbol stays resident; without runs no symbol is derived: a one-hot row for the dominant one too
        assert store.plane(0, 0, table.missing) is not None and store.scan_runs(0) == 0
        assert store.scan_rows(0, 3, 10) == 7 and 0 < store.scan_escapes(0) <= N_ROWS * POSITIONS // 200
    elif knob4 == 3:
        assert store.scan_rows(0, 3, 10) == 7 and store.scan_rows(0, 17, 23) == 7 and store.scan_rows(0, SECOND_FREQUENT, SECOND_FREQUENT + 1) == 2
        assert store.scan_rows(0, ALL_FREQUENT, ALL_FREQUENT + 1) > 2 and store.scan_rows(0, 12, 13) == 2 and store.scan_rows(0, 0, 3) == 6
        assert 0 < store.scan_escapes(0) <= N_ROWS * POSITIONS // 200
    elif knob4 == 2:
        assert store.scan_planes(0) == 2
        assert 2 * POSITIONS < store.scan_rows(0, 0, POSITIONS) <= 2 * (POSITIONS - 1) + full_planes
        assert store.scan_rows(0, ALL_FREQUENT, ALL_FREQUENT + 1) > 2 and store.scan_rows(0, 12, 13) == 2
        assert 0 < store.scan_escapes(0) <= N_ROWS * POSITIONS // 200
    else:
        assert store.scan_planes(0) == full_planes and store.scan_rows(0, 0, POSITIONS) == full_planes * POSITIONS
        assert store.scan_escapes(0) == 0


@functools.lru_cache(maxsize=None)
def _ranges():
    """N_RANGES weeks from day 1000 on, in a shuffled request order."""
    rng = np.random.default_rng(31)
    return tuple((1000 + 7 * int(k), 1006 + 7 * int(k)) for k in rng.permutation(N_RANGES))


def _distinct_ranges_per_word(groups):
    """(distinct range ids per word of 64 rows, whether the word has rows in no range)."""
    padded = np.full(-(-len(groups) // 64) * 64, NO_GROUP, dtype=np.uint16)
    padded[:len(groups)] = groups
    words = np.sort(padded.reshape(-1, 64), axis=1)
    has_none = words[:, -1] == NO_GROUP
    return (np.diff(words.astype(np.int64), axis=1) != 0).sum(axis=1) + 1 - has_none, has_none


@functools.lru_cache(maxsize=None)
def _date_columns():
    """Three columns over N_ROWS: dates sorted in blocks (words of one or two ranges: the segment path), uniformly random dates
    (every word goes row by row), and a constructed one where word w holds exactly w % 7 + 1 distinct ranges, every third word
    with NULL and out-of-range rows between them."""
    rng = np.random.default_rng(32)
    ranges = _ranges()
    everyone = np.ones(N_ROWS, bool)
    blocks = np.concatenate([np.sort(rng.integers(990, 1000 + 7 * N_RANGES + 10, size=size)) for size in np.diff(np.linspace(0, N_ROWS, 31).astype(int))])
    scattered = rng.choice(N_ROWS, size=N_ROWS // 200, replace=False)
    blocks[scattered] = rng.integers(990, 1000 + 7 * N_RANGES + 10, size=len(scattered))
    blocks[rng.choice(N_ROWS, size=500, replace=False)] = 0
    uniform = 1000 + rng.integers(0, 7 * N_RANGES, size=N_ROWS)
    uniform[rng.random(N_ROWS) < 0.01] = 0
    uniform[rng.random(N_ROWS) < 0.01] = 5
    n_words = -(-N_ROWS // 64)
    built = np.zeros(n_words * 64, dtype=np.int64)
    for w in range(n_words):
        k = w % 7 + 1
        ids = rng.choice(N_RANGES, size=k, replace=False)
        fill = rng.choice(ids, size=64 - k)
        dates = np.array([ranges[g][0] for g in np.concatenate([ids, fill])]) + rng.integers(0, 7, size=64)
        if w % 3 == 1:
            unset = k + rng.choice(64 - k, size=12, replace=False)
            dates[unset[:6]], dates[unset[6:]] = 0, 5
        built[64 * w:64 * w + 64] = rng.permutation(dates)
    built = built[:N_ROWS]
    columns = [blocks.astype(np.uint32), uniform.astype(np.uint32), built.astype(np.uint32)]
    # not vacuous: the second column has words of more than 4 ranges, the third has words of exactly 4 and exactly 5, with and
    # without rows in no range; most words of the first stay within the 4 segments
    distinct, has_none = zip(*[_distinct_ranges_per_word(dense.row_groups(everyone, column, ranges)) for column in columns])
    assert (distinct[0] <= 4).mean() > 0.9 and (distinct[0] >= 2).any()
    assert (distinct[1] > 4).mean() > 0.99
    full_words = N_ROWS // 64
    assert np.array_equal(distinct[2][:full_words], np.arange(full_words) % 7 + 1)
    for exactly in (4, 5):
        assert ((distinct[2] == exactly) & has_none[2]).any() and ((distinct[2] == exactly) & ~has_none[2]).any()
    for column in columns:
        column.setflags(write=False)
    return columns


@functools.lru_cache(maxsize=None)
def _all_cells(alphabet):
    """Every valid symbol at each listed position."""
    return tuple((p, s) for p in LISTED_POSITIONS for s in _alphabet(alphabet).valid_mutation_symbols)


def _mutation_lists(alphabet):
    """All valid symbols at the listed positions; that list shuffled, with duplicates; lists of 1, 16, 17 and 33 cells in which
    position 5 (derived under knob 4 = 0) stands at index 0, 16 and 32: in three blocks of 16 mutations."""
    rng = np.random.default_rng(33)
    cells = list(_all_cells(alphabet))
    shuffled = cells + [cells[k] for k in rng.integers(0, len(cells), size=10)]
    shuffled = [shuffled[k] for k in rng.permutation(len(shuffled))]
    valid = list(_alphabet(alphabet).valid_mutation_symbols)
    elsewhere = [cell for cell in shuffled if cell[0] != 5]
    short = [elsewhere[k % len(elsewhere)] for k in range(33)]
    short[0], short[16], short[32] = (5, valid[1]), (5, valid[2]), (5, valid[1])
    short[3], short[20] = (ABSENT_AT, valid[0]), (ABSENT_AT, valid[3])  # a second derived position on both sides of index 16
    assert len({position for position, _ in short}) >= 5
    return [cells, shuffled, short[:1], short[:16], short[:17], short]


@functools.lru_cache(maxsize=None)
def _filters():
    rng = np.random.default_rng(34)
    nine = np.zeros(N_ROWS, bool)
    nine[rng.choice(N_ROWS, size=9, replace=False)] = True
    clustered = (np.arange(N_ROWS) >= int(N_ROWS * 0.6)) & (rng.random(N_ROWS) < 0.7)
    return [None, rng.random(N_ROWS) < 0.4, nine, clustered]


def _reference_by_cell(alphabet, mask, dates):
    """{cell: uint32 [G][2]} for every valid symbol at every listed position, computed once per (filter, date column)."""
    cells = _all_cells(alphabet)
    mask = np.ones(N_ROWS, bool) if mask is None else mask
    table = dense.grouped_mutation_counts(_matrix(alphabet), mask, dates, _ranges(), cells, _alphabet(alphabet).valid_mutation_symbols)
    return dict(zip(cells, table))


def _expected(by_cell, cells):
    return np.stack([by_cell[cell] for cell in cells])


def test_the_listed_cells_cover_every_kind():
    """What (b) lists, in numpy: an absent symbol, symbols with a handful of rows at a settled position (escape keys there once
    its dominant symbol is derived), the dominant symbols themselves, rows without a valid symbol at every listed position."""
    for alphabet in ("nuc", "aa"):
        sym, table = _matrix(alphabet), _alphabet(alphabet)
        valid = list(table.valid_mutation_symbols)
        counts = dense.mutation_counts(sym, np.ones(N_ROWS, bool), valid)
        assert (counts[ABSENT_AT] == 0).sum() >= 1
        for position in (5, ABSENT_AT):
            assert counts[position].max() > 0.95 * N_ROWS and ((counts[position] > 0) & (counts[position] < 50)).any()
        assert (counts[ALL_FREQUENT] > N_ROWS // 40).all()
        for position in LISTED_POSITIONS:
            assert (sym[:, position] == table.missing).sum() > 150 and (~np.isin(sym[:, position], valid + [table.missing])).any()


@pytest.mark.parametrize("knob4,knob8", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_grouped_counts_in_every_layout(built, alphabet, knob4, knob8):
    """Every cell of silo_gpu_mutations_grouped against numpy: 5 layouts x 2 alphabets, 3 date columns (segment path, row by row,
    exactly 1..7 ranges per word), 4 filters, 6 mutation lists.  Per (filter, date column) also: the counts of a position's valid
    symbols add up to its coverage in every range, and three ranges equal silo_gpu_mutations_scan under And(filter, range)."""
    sym, table = _matrix(alphabet), _alphabet(alphabet)
    valid = list(table.valid_mutation_symbols)
    ranges = _ranges()
    lists = _mutation_lists(alphabet)
    n_valid = len(valid)
    with _layout_store(alphabet, knob4, knob8) as store:
        _assert_layout(store, alphabet, knob4, knob8)
        scan_symbols = list(store.scan_symbols[0])
        assert scan_symbols == valid
        filters = [(mask, _upload_mask(store, mask)) for mask in _filters()]
        scan_filter = store.bitset_alloc()
        for column_index, dates in enumerate(_date_columns()):
            dates_dev = store.upload_column(dates)
            for filter_index, (mask, filter_ptr) in enumerate(filters):
                where = (alphabet, knob4, knob8, column_index, filter_index)
                by_cell = _reference_by_cell(alphabet, mask, dates)
                for list_index, cells in enumerate(lists):
                    got = _grouped(store, filter_ptr, dates_dev, ranges, cells)
                    assert got.shape == (len(cells), N_RANGES, 2)
                    assert np.array_equal(got, _expected(by_cell, cells)), where + (list_index,)
                    if list_index == 0:
                        per_position = got.reshape(len(LISTED_POSITIONS), n_valid, N_RANGES, 2)
                        assert np.array_equal(per_position[:, :, :, 0].sum(axis=1), per_position[:, 0, :, 1]), where
                        assert (per_position[:, :, :, 1] == per_position[:, :1, :, 1]).all(), where
                        for g in (0, 17, N_RANGES - 1):
                            selected = (np.ones(N_ROWS, bool) if mask is None else mask) & _in_range(dates, *ranges[g])
                            store.bitset_upload(scan_filter, dense.pack_bits(selected))
                            scan = store.mutations_scan(0, scan_filter)
                            assert np.array_equal(got[:, g, 0], [scan[p][valid.index(s)] for p, s in cells]), where + (g,)
                            assert np.array_equal(got[:, g, 1], [scan[p].sum() for p, _ in cells]), where + (g,)
                if mask is None:
                    assert got[:, :, 0].any()
            store.free(dates_dev)


# ---- c: limits -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def derived_store(built):
    """The nucleotide store of (b) with its dominant symbols derived and the missing symbol as runs."""
    store = _layout_store("nuc", 0, 0)
    _assert_layout(store, "nuc", 0, 0)
    yield store
    store.close()


def test_1024_ranges_and_4096_mutations(derived_store):
    """G = 1 024 x M = 17 (the LDS histograms of k_assign_groups and k_grouped_position_counts are strided over by 256 threads; once
    with sorted dates: segments, once with random ones: row by row) and G = 3 x M = 4 096 (256 blocks of mutations): every cell."""
    store, sym = derived_store, _matrix("nuc")
    rng = np.random.default_rng(35)
    valid = [0, 1, 2, 3, 4]
    everyone = np.ones(N_ROWS, bool)
    cells = list(_all_cells("nuc"))
    seventeen = [cells[k] for k in rng.permutation(len(cells))[:17]]
    seventeen[0], seventeen[16] = (5, 1), (5, 3)
    days = [(3000 + int(k), 3000 + int(k)) for k in rng.permutation(1024)]
    random_dates = rng.integers(2990, 4034, size=N_ROWS).astype(np.uint32)
    mask = rng.random(N_ROWS) < 0.6
    filter_ptr = _upload_mask(store, mask)
    for dates, selected, ptr in ((np.sort(random_dates), everyone, None), (random_dates, mask, filter_ptr)):
        dates_dev = store.upload_column(dates)
        got, groups = _grouped(store, ptr, dates_dev, days, seventeen, return_groups=True)
        assert np.array_equal(groups[:N_ROWS], dense.row_groups(selected, dates, days))
        want = dense.grouped_mutation_counts(sym, selected, dates, days, seventeen, valid)
        assert want[:, :, 0].any() and (want[:, :, 1] > 0).all(axis=0).sum() > 1000
        assert np.array_equal(got, want)
        store.free(dates_dev)
    three = [(1000, 1100), (1200, UNBOUNDED), (0, 999)]
    many = [cells[k % len(cells)] for k in range(4096)]
    dates = _date_columns()[1]
    dates_dev = store.upload_column(dates)
    by_cell = dict(zip(cells, dense.grouped_mutation_counts(sym, mask, dates, three, cells, valid)))
    got = _grouped(store, filter_ptr, dates_dev, three, many)
    assert got.shape == (4096, 3, 2)
    assert np.array_equal(got, _expected(by_cell, many))
    store.free(dates_dev)


def test_more_than_the_limits_is_refused(derived_store):
    from silo_amd.binding import MAX_DATE_RANGES, MAX_GROUPED_MUTATIONS, SiloGpuError

    store = derived_store
    dates_dev = store.upload_column(_date_columns()[0])
    days = [(3000 + k, 3000 + k) for k in range(MAX_DATE_RANGES + 1)]
    with pytest.raises(SiloGpuError) as refusal:
        _grouped(store, None, dates_dev, days, [(5, 1)])
    assert refusal.value.code < 0
    with pytest.raises(SiloGpuError) as refusal:
        _grouped(store, None, dates_dev, days[:2], [(5, 1)] * (MAX_GROUPED_MUTATIONS + 1))
    assert refusal.value.code < 0
    _check_a_valid_call(store, dates_dev)
    store.free(dates_dev)


def test_4096_derived_positions(built):
    """k_grouped_missing_runs with its LDS table full: one mutation at each of 4 096 distinct derived positions of a store of
    4 100 settled positions whose rows carry runs of N.  (63 490 rows: finalize re-encodes a store, and so derives a symbol, from
    1 024 row words on.)"""
    rng = np.random.default_rng(36)
    n, positions = 63_490, 4100
    dominant = rng.integers(1, 5, size=positions).astype(np.uint8)
    sym = np.broadcast_to(dominant, (n, positions)).copy()
    other = rng.integers(0, n * positions, size=n * positions // 800)  # other valid symbols, ambiguity codes, single N cells
    sym.reshape(-1)[other] = rng.integers(0, 16, size=len(other))
    for row in rng.choice(n, size=3000, replace=False):
        start = int(rng.integers(0, positions))
        sym[row, start:start + int(rng.geometric(0.01))] = 15
    sym[rng.choice(n, size=5, replace=False), :] = 15
    sym[7, 0], sym[8, positions - 1] = 15, 15
    with make_store(n, [dict(name="a", alphabet="nuc", reference=dominant)]) as store:
        store.tune(9, -1)
        try:
            store.append_sequences(0, 0, NUC_CHARS[sym])
            store.finalize()
        finally:
            store.tune(9, 0)
        assert store.scan_rows(0, 0, positions) == 0 and store.scan_runs(0) > 3000  # every position derived, the missing symbol as runs
        # 4 096 distinct positions, the first and the last position of the store among them, in no order
        listed = rng.permutation(np.concatenate([[0, positions - 1], rng.permutation(np.arange(1, positions - 1))[:4094]]))
        symbols = np.where(rng.random(4096) < 0.6, dominant[listed], rng.integers(0, 5, size=4096))
        cells = list(zip(listed.tolist(), symbols.tolist()))
        assert len({p for p, _ in cells}) == 4096
        dates = rng.integers(0, 160, size=n).astype(np.uint32)
        ranges = [(40, 49), (1, 9), (10, 25)]
        dates_dev = store.upload_column(dates)
        mask = rng.random(n) < 0.5
        for selected, ptr in ((np.ones(n, bool), None), (mask, _upload_mask(store, mask))):
            want = dense.grouped_mutation_counts(sym, selected, dates, ranges, cells, [0, 1, 2, 3, 4])
            cardinality = np.bincount(dense.row_groups(selected, dates, ranges), minlength=3)[:3]
            assert (want[:, :, 1] < cardinality).any(axis=1).mean() > 0.9 and want[:, :, 0].any()  # rows without a symbol at most positions
            assert np.array_equal(_grouped(store, ptr, dates_dev, ranges, cells), want)
        store.free(dates_dev)


# ---- d: accumulation -------------------------------------------------------------------------------------------------------------
def test_the_table_is_accumulated_into(derived_store):
    """Two calls with different filters into one table that starts out as random numbers: start + A + B; a call without ranges or
    without mutations succeeds and leaves the table as it is."""
    store, sym = derived_store, _matrix("nuc")
    rng = np.random.default_rng(37)
    cells = _mutation_lists("nuc")[5]
    ranges = _ranges()
    dates = _date_columns()[2]
    dates_dev = store.upload_column(dates)
    masks = [rng.random(N_ROWS) < 0.3, np.arange(N_ROWS) % 5 == 1]
    start = rng.integers(1, 1 << 20, size=(len(cells), N_RANGES, 2)).astype(np.uint32)
    table_dev = store.upload_column(start.reshape(-1))
    want = start.copy()
    for mask in masks:
        assert _grouped(store, _upload_mask(store, mask), dates_dev, ranges, cells, out_ptr=table_dev) is None
        want += dense.grouped_mutation_counts(sym, mask, dates, ranges, cells, [0, 1, 2, 3, 4])
    assert np.array_equal(store.read(table_dev, np.uint32, start.size).reshape(start.shape), want)
    assert (want != start).any()
    assert _grouped(store, None, dates_dev, [], cells, out_ptr=table_dev) is None
    assert _grouped(store, None, dates_dev, ranges, [], out_ptr=table_dev) is None
    assert np.array_equal(store.read(table_dev, np.uint32, start.size).reshape(start.shape), want)
    assert _grouped(store, None, dates_dev, [], cells).shape == (len(cells), 0, 2)
    assert _grouped(store, None, dates_dev, ranges, []).shape == (0, N_RANGES, 2)
    store.free(table_dev)
    store.free(dates_dev)


# ---- e: refusals -----------------------------------------------------------------------------------------------------------------
def _check_a_valid_call(store, dates_dev, column=0):
    cells = _mutation_lists("nuc")[4]
    want = dense.grouped_mutation_counts(_matrix("nuc"), np.ones(N_ROWS, bool), _date_columns()[column], _ranges(), cells, [0, 1, 2, 3, 4])
    assert np.array_equal(_grouped(store, None, dates_dev, _ranges(), cells), want)


def test_refusals_at_the_entry(derived_store):
    """from > to, overlapping ranges, ranges that share a day, a position past the last, the missing symbol, an ambiguity code and
    a null scratch are refused with an error status; the next valid call on the store answers exactly."""
    from silo_amd.binding import SiloGpuError

    store = derived_store
    dates_dev = store.upload_column(_date_columns()[0])
    good_ranges, good_cells = [(1000, 1006), (1007, 1013)], [(5, 1), (ALL_FREQUENT, 2)]
    refused = [
        ([(1006, 1000)], good_cells, {}),
        ([(1000, 1010), (1005, 1020)], good_cells, {}),
        ([(1020, 1030), (1000, 1025)], good_cells, {}),   # overlapping, given in descending order
        ([(1000, 1006), (1006, 1013)], good_cells, {}),   # to == the next from: both ends are inclusive
        ([(0, 1006), (0, 0)], good_cells, {}),
        (good_ranges, [(5, 1), (POSITIONS, 1)], {}),
        (good_ranges, [(5, 15)], {}),                     # N
        (good_ranges, [(5, 1), (5, 5)], {}),              # R
        (good_ranges, [(5, 16)], {}),                     # no symbol of the alphabet
        (good_ranges, good_cells, dict(scratch_ptr=None)),
    ]
    for ranges, cells, options in refused:
        with pytest.raises(SiloGpuError) as refusal:
            _grouped(store, None, dates_dev, ranges, cells, **options)
        assert refusal.value.code < 0, (ranges, cells, options)
        _check_a_valid_call(store, dates_dev)
    with pytest.raises(SiloGpuError):
        store.mutations_grouped(1, None, dates_dev, good_ranges, [5], [1])  # no such sequence store
    _check_a_valid_call(store, dates_dev)
    store.free(dates_dev)


def test_a_sequence_store_without_sequences_is_refused(built):
    from silo_amd.binding import SiloGpuError

    rng = np.random.default_rng(38)
    n = 2049
    sym = rng.integers(0, 5, size=(n, 3)).astype(np.uint8)
    dates = rng.integers(0, 30, size=n).astype(np.uint32)
    ranges, cells = [(1, 9), (10, 40)], [(0, 1), (2, 0), (1, 4)]
    with make_store(n, [dict(name="a", alphabet="nuc", reference=np.ones(3, dtype=np.uint8))]) as store:
        dates_dev = store.upload_column(dates)
        with pytest.raises(SiloGpuError) as refusal:
            _grouped(store, None, dates_dev, ranges, cells)
        assert refusal.value.code < 0
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        want = dense.grouped_mutation_counts(sym, np.ones(n, bool), dates, ranges, cells, [0, 1, 2, 3, 4])
        assert want[:, :, 0].all()
        assert np.array_equal(_grouped(store, None, dates_dev, ranges, cells), want)
        store.free(dates_dev)
