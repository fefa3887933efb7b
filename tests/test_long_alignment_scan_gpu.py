"""The Mutations scan over derived stores of MORE positions than one turn of the finish kernel's prefix sweep covers.  A block of
k_finish_scan sums the gap events (and end events) of all positions before its own, 4 x 1 024 16-byte loads a turn: two
positions of events each, so a block whose first position lies beyond 8 192 takes a second turn — a range of more than 9 216
positions — and, without gap events (four positions of diff a load), one beyond 16 384: more than 17 408 positions.  The genome
this project is for has 29 903.  Every table against oracle.dense.mutation_counts, summed over chunks of rows as the store is
filled: the whole matrix is never held."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import scan_alignments as sa  # noqa: E402
from tests.scan_alignments import GAP  # noqa: E402

N = 65_600       # the fewest rows whose store is re-encoded (rows of at least one column tile): one slice of rows and 64 more
CHUNK = 8_200    # rows generated, counted by the oracle and appended at a time
FINISH_BLOCK = 1_024
FILTERS = ["random 40 %", "all rows", "a few hundred rows", "empty", "rows >= 60 %", "random 90 %", "the last 64 rows", "70 % of the first 60 %"]


class Built:
    pass


def frequent_positions(positions, first_turn):
    """Positions where the second symbol has 8 % or 60 % of the rows — reported at 0.05 / at 0.5 —: the first and last threads of
    finish blocks on either side of the sweep's first turn."""
    last_block = (positions - 1) // FINISH_BLOCK * FINISH_BLOCK
    return {150: 0.08, 4_095: 0.6, 4_096: 0.08, first_turn - 1: 0.08, first_turn: 0.6, last_block - 1: 0.08, last_block: 0.6, last_block + 40: 0.08}


def fill(rng, symbols, reference, second, first_turn, classes, store=None):
    """Generates the alignment chunk by chunk — the reference sequence plus exceptions —, adds each chunk's oracle tables to the
    expected ones and appends it to `store` (None: a dry run of the host side)."""
    positions = len(reference)
    last_block = (positions - 1) // FINISH_BLOCK * FINISH_BLOCK
    frequent = frequent_positions(positions, first_turn)
    scan_symbols = symbols.valid.tolist()
    want = {name: np.zeros((positions, symbols.n_scan), dtype=np.uint32) for name in FILTERS}
    every_97th = np.arange(0, positions, 97)
    seen = dict(sweep_runs=0, sweep_trails=0)
    for first_row in range(0, N, CHUNK):
        n_rows = min(CHUNK, N - first_row)
        chunk = np.tile(reference, (n_rows, 1))
        chunk[rng.integers(0, n_rows, size=(len(every_97th), 3)), every_97th[:, None]] = second[every_97th][:, None]  # a few valid mutations
        for position, share in frequent.items():
            chunk[rng.random(n_rows) < share, position] = second[position]
        rows = rng.permutation(n_rows)
        ragged, long_trails, with_runs, whole = rows[:int(0.7 * n_rows)], rows[-200:-170], rows[-170:-50], rows[-50:-48]
        sa.add_ragged_ends(rng, chunk, ragged, 30, 30, 400)
        for row in long_trails:  # trailing runs that begin behind the sweep's first turn and before the last finish block
            chunk[row, int(rng.integers(first_turn + 4, last_block - 4)):] = GAP
        sa.add_missing_runs(rng, symbols, chunk, with_runs, 300, crossing=[
            ((3_000, 4_090), (4_100, 6_000), 15), ((first_turn - 600, first_turn - 2), (first_turn + 2, first_turn + 600), 15),
            ((first_turn + 8, last_block - 16), (last_block + 4, positions), 20)])  # the last: begun in the second turn's part, open in the last block
        sa.add_lone_codes(rng, symbols, chunk, rows[:-50], 3_000)
        if first_row == 0:  # one row of each throughout (more rows of '-' would be a key at every position: no granule would get wide)
            chunk[whole[0]], chunk[whole[1]] = symbols.missing, GAP
        seen["sweep_runs"] += int(((chunk[:, last_block] == symbols.missing) & (chunk[:, first_turn] != symbols.missing)).sum())
        seen["sweep_trails"] += len(long_trails)
        for name, table in classes.oracle_tables(chunk, scan_symbols, first_row).items():
            want[name] += table
        if store is not None:
            store.append_sequences(0, first_row, symbols.chars[chunk])
    made = Built()
    made.symbols, made.positions, made.first_turn, made.last_block, made.frequent, made.seen = symbols, positions, first_turn, last_block, frequent, seen
    made.reference, made.second, made.want = reference, second, want
    made.reference_index = sa.reference_index(scan_symbols, reference)
    made.never_pruned = np.flatnonzero(want["all rows"].argmax(axis=1) != made.reference_index).tolist()
    return made


def row_classes(rng):
    rows = np.arange(N)
    share = np.digitize(rng.random(N), [0.005, 0.4, 0.7, 0.9])
    region = np.where(rows >= 65_536, 2, np.where(rows >= int(0.6 * N), 1, 0))
    classes = sa.RowClasses(share * 3 + region)
    classes.add("random 40 %", lambda label: label // 3 <= 1)
    classes.add("all rows", lambda label: True)
    classes.add("a few hundred rows", lambda label: label // 3 == 0)
    classes.add("empty", lambda label: False)
    classes.add("rows >= 60 %", lambda label: label % 3 >= 1 and label // 3 <= 2)
    classes.add("random 90 %", lambda label: label // 3 <= 3)
    classes.add("the last 64 rows", lambda label: label % 3 == 2)
    classes.add("70 % of the first 60 %", lambda label: label % 3 == 0 and label // 3 <= 2)
    assert classes.names() == FILTERS
    return classes


def filled_store(alphabet, positions, first_turn, seed):
    """A generator of one finalized store of the alignment with its filters uploaded and what the oracle expects of it."""
    from silo_amd.binding import GpuStore

    rng = np.random.default_rng(seed)
    symbols = sa.Symbols(alphabet)
    classes = row_classes(rng)
    reference, second, _ = sa.symbol_orders(rng, symbols, positions)
    with GpuStore(N, [dict(name="main", alphabet=alphabet, reference=reference.copy())]) as store:
        store.tune(sa.TUNE_LAUNCH_COST, -1)  # (no charge per kind of launch: a small store is to derive symbols too)
        try:
            made = fill(rng, symbols, reference, second, first_turn, classes, store)
            store.finalize()
        finally:
            store.tune(sa.TUNE_LAUNCH_COST, 0)
        made.store = store
        made.filters = dict(zip(FILTERS, sa.upload(store, [classes.mask(name) for name in FILTERS])))
        made.masks = {name: classes.mask(name) for name in FILTERS}
        yield made


@pytest.fixture(scope="module")
def nucleotides(built):
    yield from filled_store("nuc", 9_300, 8_192, 211)


@pytest.fixture(scope="module")
def amino_acids(built):
    yield from filled_store("aa", 9_300, 8_192, 223)


@pytest.fixture(scope="module")
def long_nucleotides(built):
    yield from filled_store("nuc", 17_500, 16_384, 227)


def check_preconditions(made):
    """On the oracle's side: runs of the missing symbol that begin behind the sweep's first turn and are open in the last finish
    block, trailing runs that begin there, settled positions.  On the store's: derived symbols, overflow keys, end runs."""
    store, positions = made.store, made.positions
    assert positions > made.last_block > made.first_turn + FINISH_BLOCK - 1  # the last block's sweep takes a second turn
    assert made.seen["sweep_runs"] >= 100 and made.seen["sweep_trails"] >= 100
    total = made.want["all rows"]
    assert (total.argmax(axis=1) == made.reference_index).mean() > 0.95
    assert total[made.last_block + 10, 0] > made.seen["sweep_trails"]  # '-' in the last block: the ragged ends
    assert store.scan_runs(0) > 0
    assert store.scan_overflow_keys(0) > 0  # a few keys per 97 positions: granules far wider than the escape pass's window
    covered, events, _ = store.scan_end_runs(0)
    assert covered > 0 and events > 0


def ranges_of(made):
    """The whole store, and sub-ranges that begin at 0, 4 095 / 4 096, around the first turn's end and around the last block's
    first position.  The sweep runs over the RANGE's positions (a block's first position counts from the range's), so only
    ranges of more than first_turn + 1 024 positions take the second turn: the first three."""
    p, turn, last = made.positions, made.first_turn, made.last_block
    ranges = [(0, 0, p), (0, 0, last + 34), (0, 50, p - 1), (0, 4_095, p), (0, 4_096, last), (0, turn - 1, last + 1), (0, turn, p), (0, last - 1, p), (0, last, p)]
    assert [b - a > turn + FINISH_BLOCK for _, a, b in ranges] == [True] * 3 + [False] * 6
    return ranges


def check_exact(made, q_counts, ranges, settings):
    store = made.store
    for q_count in q_counts:
        names = FILTERS[:q_count]
        tables, kernels = sa.timed(store, settings, lambda: store.mutations_scan_ranges(ranges, [made.filters[name] for name in names]))
        sa.check_kernels(kernels, q_count, settings.get(sa.TUNE_GAP_EVENTS, 0), 0)
        for (_, a, b), per_filter in zip(ranges, tables):
            for name, table in zip(names, per_filter):
                assert np.array_equal(table, made.want[name][a:b]), (a, b, name)


def check_pruned(made, q_counts, ranges, proportion=0.05):
    store = made.store
    cardinality = int(made.masks["random 40 %"].sum())
    assert store.scan_prunable_granules(0, cardinality, proportion)[0] > 0
    for q_count in q_counts:
        names = FILTERS[:q_count]
        tables, kernels = sa.timed(store, {}, lambda: store.mutations_scan_ranges(ranges, [made.filters[name] for name in names], min_proportions=[proportion] * q_count))
        assert any(", pruning" in k for k in kernels), kernels
        for (_, a, b), per_filter in zip(ranges, tables):
            never = [p - a for p in made.never_pruned if a <= p < b]
            for name, pruned in zip(names, per_filter):
                sa.check_pruned(store, pruned, made.want[name][a:b], made.reference_index[a:b], proportion, never, (a, b, name))
        if q_count == 1:  # (something was left out; with the empty filter in the launch nothing may be)
            assert not np.array_equal(tables[0][0], made.want[FILTERS[0]][ranges[0][1]:ranges[0][2]])


def check_fused_select(made, q_counts, proportions=(0.05, 0.5)):
    from silo_amd import binding

    store, positions, n_scan = made.store, made.positions, made.symbols.n_scan
    reference = np.ascontiguousarray(made.reference_index)
    reference_dev = ctypes.c_void_p()
    assert store.lib.silo_gpu_upload_bytes(reference.ctypes.data_as(ctypes.c_void_p), reference.nbytes, ctypes.byref(reference_dev)) == 0
    slots = [binding.RowSlot(16_384) for _ in range(max(q_counts))]
    tables = [store.malloc(4 * positions * n_scan) for _ in range(max(q_counts))]
    try:
        for q_count in q_counts:
            names = FILTERS[:q_count]
            for proportion in proportions:
                for table in tables[:q_count]:
                    store.memset(table, 0xA5, 4 * positions * n_scan)
                _, kernels = sa.timed(store, {}, lambda: store.mutations_scan_select(
                    [(0, 0, positions)], [made.filters[name] for name in names], [proportion] * q_count, tables[:q_count], [0], positions, reference_dev, slots[:q_count]))
                assert "k_finish_scan<true, %u>" % n_scan in kernels, kernels
                for name, table_dev, slot in zip(names, tables, slots):
                    n_selected, rows = slot.wait()
                    want_rows = sa.oracle_rows(made.want[name], made.reference_index, proportion)
                    assert (n_selected, sorted(map(tuple, rows.tolist()))) == (len(want_rows), want_rows), (name, proportion)
                    table = store.read(table_dev, np.uint32, positions * n_scan).reshape(positions, n_scan)
                    assert np.array_equal(table.sum(axis=1, dtype=np.uint32), made.want[name].sum(axis=1, dtype=np.uint32)), (name, proportion)
                    never = np.asarray(made.never_pruned, dtype=np.int64)
                    assert np.array_equal(table[never], made.want[name][never]), (name, proportion)
                    if name in ("random 40 %", "all rows"):  # (not vacuous: the frequent second symbols beyond the first turn are reported)
                        reported = {row[0] for row in want_rows}
                        assert reported >= {p for p, share in made.frequent.items() if share > 1.2 * proportion and p >= made.first_turn}
    finally:
        for slot in slots:
            slot.close()
        store.lib.silo_gpu_free(reference_dev)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_two_turns_of_the_event_sweep(alphabet, request):
    """9 300 positions, gap events and end events: the finish block of positions 9 216 to 9 299 sums the events of 9 216
    positions, 4 608 loads of 16 bytes for 4 096 places a turn.  Exact tables of the whole store and of sub-ranges for 1, 2 and 8
    filters, the pruning entry at 0.05, and the scan that selects its rows in the finish kernel."""
    made = request.getfixturevalue("nucleotides" if alphabet == "nuc" else "amino_acids")
    check_preconditions(made)
    ranges = ranges_of(made)
    check_exact(made, (1, 2, 8), ranges, {sa.TUNE_GAP_EVENTS: 0})
    check_pruned(made, (1, 8), [ranges[0], ranges[2], ranges[6]])
    check_fused_select(made, (1, 2, 8))


def test_two_turns_of_the_sweep_without_gap_events(long_nucleotides):
    """17 500 positions with SILO_GPU_TUNE_GAP_EVENTS = -1: the runs of the missing symbol counted into one diff per position,
    four positions a load — the block of positions 17 408 to 17 499 sums 4 352 loads.  One scan of the whole store, two filters."""
    made = long_nucleotides
    assert made.store.scan_runs(0) > 0 and made.seen["sweep_runs"] >= 100
    assert made.positions > made.last_block > made.first_turn + FINISH_BLOCK - 1
    check_exact(made, (2,), [(0, 0, made.positions)], {sa.TUNE_GAP_EVENTS: -1})
