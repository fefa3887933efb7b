"""silo_gpu_mutations_scan_select: the Mutations scan that overwrites its count tables and delivers the selected rows into row
slots — where the call allows it, inside the finish kernel of the scan (k_finish_scan<true, n_scan>).  Tables and rows against the
dense oracle with the threshold arithmetic in numpy, and against the route through the other entries on the same store
(silo_gpu_mutations_scan_ranges_min_proportion into a cleared table, then silo_gpu_mutations_select_to_slot)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
GAP, N_SYMBOL = 0, 15
TUNE_SCAN_TIMING, TUNE_FUSED_SELECT = 7, 13

# At least 65 536 rows: finalize chooses derived layouts.  More than 2 x 1 024 positions and no multiple of 1 024: the finish launch
# has three blocks, the last partial.
N, POSITIONS = 66_000, 2_100
FINISH_BLOCK = 1_024
CAPACITY = 16_384  # more than the 4 x 2 100 cells a proportion of 0 can select
PROPORTIONS = [0.0, 0.05, 0.5, 1.0]
FILTERS = ["random 40 %", "all rows", "no row", "3 rows"]
# positions where a second symbol has 8 % / 60 % of the rows (reported at 0.05 / at 0.5): the first and last threads of every block
FREQUENT = {0: 0.08, 1_023: 0.6, 1_024: 0.08, 1_500: 0.6, 2_047: 0.08, 2_048: 0.6, 2_099: 0.08, 700: 0.08}


class Built:
    pass


def ragged_alignment(rng, n, positions, end_mean=300):
    """One of A, C, G, T in nearly every row of a position, a second one in 0.02 % of them (FREQUENT: more), other symbols — the
    ambiguity codes and N — in 0.1 %, generated in chunks of positions; leading and trailing runs of '-' of geometric length in
    97 % of the rows; runs of N; a few rows of N throughout."""
    dominant = rng.integers(1, 5, size=positions).astype(np.uint8)
    second = ((dominant % 4) + 1).astype(np.uint8)
    sym = np.empty((n, positions), dtype=np.uint8)
    for a in range(0, positions, 300):
        b = min(a + 300, positions)
        draw = rng.random((n, b - a), dtype=np.float32)
        share = np.array([FREQUENT.get(p, 0.0002) for p in range(a, b)], dtype=np.float32)
        chunk = np.where(draw < share[None, :], second[None, a:b], dominant[None, a:b]).astype(np.uint8)
        lone = (draw >= share[None, :]) & (draw < share[None, :] + 0.001)
        chunk[lone] = rng.integers(5, 16, size=int(lone.sum()))
        sym[:, a:b] = chunk
    lead = np.where(rng.random(n) < 0.97, rng.geometric(1 / end_mean, size=n), 0)
    trail = np.where(rng.random(n) < 0.97, rng.geometric(1 / end_mean, size=n), 0)
    column = np.arange(positions)
    for a in range(0, n, 8_192):  # (chunks of rows: the comparison is rows x positions)
        sym[a:a + 8_192][column[None, :] < lead[a:a + 8_192, None]] = GAP
        sym[a:a + 8_192][column[None, :] >= positions - trail[a:a + 8_192, None]] = GAP
    rows = rng.choice(n, size=3_000, replace=False)
    for row in rows[:2_900]:  # runs of N of geometric length anywhere
        start = int(rng.integers(0, positions))
        sym[row, start:start + int(rng.geometric(1 / end_mean))] = N_SYMBOL
    for row in rows[2_900:2_950] if positions > 2_050 else []:  # ... from before position 1 024 to behind it
        sym[row, int(rng.integers(700, 1_020)):int(rng.integers(1_030, 1_400))] = N_SYMBOL
    for row in rows[2_950:] if positions > 2_050 else []:  # ... and across position 2 048
        sym[row, int(rng.integers(1_800, 2_040)):int(rng.integers(2_050, positions))] = N_SYMBOL
    sym[rng.choice(n, size=10, replace=False)] = N_SYMBOL
    return sym, dominant


def oracle_rows(table, reference, proportion):
    """The row selection of K4 (silo_gpu.h) over an exact table: sorted (position, symbol, count, total)."""
    covered = table.sum(axis=1, dtype=np.uint32)
    must_exceed = np.zeros(len(table), dtype=np.uint32)
    if proportion != 0:
        positive = covered > 0
        must_exceed[positive] = (np.ceil(covered[positive].astype(np.float64) * proportion) - 1).astype(np.uint32)
    passes = (table > must_exceed[:, None]) & (covered[:, None] > 0)
    passes[np.arange(len(table))[reference != 255], reference[reference != 255]] = False
    return sorted((int(p), int(s), int(table[p, s]), int(covered[p])) for p, s in zip(*np.nonzero(passes)))


def upload_bytes(store, array):
    array = np.ascontiguousarray(array, dtype=np.uint8)
    pointer = ctypes.c_void_p()
    assert store.lib.silo_gpu_upload_bytes(array.ctypes.data_as(ctypes.c_void_p), array.nbytes, ctypes.byref(pointer)) == 0
    return pointer


def reference_index_of(store, reference):
    scan_symbols = list(store.scan_symbols[0])
    return np.array([scan_symbols.index(s) if s in scan_symbols else 255 for s in reference], dtype=np.uint8)


@pytest.fixture(scope="module")
def data(built):
    from silo_amd import binding
    from silo_amd.binding import GpuStore

    rng = np.random.default_rng(89)
    sym, dominant = ragged_alignment(rng, N, POSITIONS)
    three = np.zeros(N, bool)
    three[[5, 40_000, N - 1]] = True
    masks = [rng.random(N) < 0.4, np.ones(N, bool), np.zeros(N, bool), three]
    made = Built()
    made.sym, made.reference, made.masks = sym, dominant, masks
    with GpuStore(N, [dict(name="main", alphabet="nuc", reference=dominant.copy())]) as store:
        for a in range(0, N, 33_000):
            store.append_sequences(0, a, NUC_CHARS[sym[a:a + 33_000]])
        store.finalize()
        store.filters = []
        for mask in masks:
            store.filters.append(store.bitset_alloc())
            store.bitset_upload(store.filters[-1], dense.pack_bits(mask))
        made.store = store
        made.reference_index = reference_index_of(store, dominant)
        made.reference_dev = upload_bytes(store, made.reference_index)
        made.slots = [binding.RowSlot(CAPACITY) for _ in range(2)]
        made.tables = [store.malloc(4 * POSITIONS * 5) for _ in range(2)]
        scan_symbols = list(store.scan_symbols[0])
        made.exact = [dense.mutation_counts(sym, mask, scan_symbols, 0, POSITIONS) for mask in masks]  # computed once, never changed
        yield made
        for slot in made.slots:
            slot.close()
        store.lib.silo_gpu_free(made.reference_dev)


def scan_select(data, filter_indexes, proportions, ranges=((0, 0, POSITIONS),), offsets=(0,), slots=None, prefill=None, knob=0, kernels=None):
    """One call of the new entry: [(table, n_selected, sorted rows)] per filter.  kernels: a list that gets the call's timing log."""
    from silo_amd import binding

    store = data.store
    slots = slots or data.slots[:len(filter_indexes)]
    tables = data.tables[:len(filter_indexes)]
    for table in tables:
        if prefill is not None:
            store.memset(table, prefill, 4 * POSITIONS * 5)
    previous = store.tune(TUNE_FUSED_SELECT, knob)
    store.tune(TUNE_SCAN_TIMING, 1 if kernels is not None else 0)
    try:
        store.mutations_scan_select(list(ranges), [store.filters[q] for q in filter_indexes], proportions, tables, list(offsets), POSITIONS,
                                    data.reference_dev, slots)
        if kernels is not None:
            kernels.extend(entry["kernel"] for entry in binding.scan_timings())
    finally:
        store.tune(TUNE_SCAN_TIMING, 0)
        store.tune(TUNE_FUSED_SELECT, previous)
    out = []
    for table, slot in zip(tables, slots):
        n_selected, rows = slot.wait()
        out.append((store.read(table, np.uint32, POSITIONS * 5).reshape(POSITIONS, 5), n_selected, sorted(map(tuple, rows.tolist()))))
    return out


def other_entries(data, filter_index, proportion, ranges=((0, 0, POSITIONS),)):
    """The same through silo_gpu_mutations_scan_ranges_min_proportion into a cleared table and silo_gpu_mutations_select_to_slot."""
    store = data.store
    table = np.zeros((POSITIONS, 5), dtype=np.uint32)
    scanned = store.mutations_scan_ranges(list(ranges), [store.filters[filter_index]], min_proportions=[proportion])
    for (_, a, b), per_filter in zip(ranges, scanned):
        table[a:b] = per_filter[0]
    n_selected, rows = store.mutations_select_to_slot(table, data.reference_index, proportion, data.slots[1])
    return table, n_selected, sorted(map(tuple, rows.tolist()))


def test_the_store_derives_symbols_and_counts_gap_and_end_events(data):
    from silo_amd import binding

    store = data.store
    assert store.scan_runs(0) > 0  # derived symbols, N kept as runs
    covered, events, residual = store.scan_end_runs(0)
    print("covered rows", covered, "end events", events, "residual keys", residual)
    assert covered > 0 and events > 0
    store.tune(TUNE_SCAN_TIMING, 1)
    try:
        store.mutations_scan_ranges([(0, 0, POSITIONS)], [store.filters[0]])
        kernels = [entry["kernel"] for entry in binding.scan_timings()]
    finally:
        store.tune(TUNE_SCAN_TIMING, 0)
    assert any(k.startswith("k_scan_escapes_sliced<") for k in kernels), kernels  # the gap events: one more range of the escape pass ...
    assert not any(k.startswith(("k_scan_missing_runs", "k_count_sparse_keys")) for k in kernels), kernels  # ... and no pass over the runs
    # covered positions on both sides of the finish launch's block borders
    gap_share = (data.sym == GAP).mean(axis=0)
    assert gap_share[FINISH_BLOCK - 5] > 0.01 and gap_share[FINISH_BLOCK + 5] > 0.01
    assert gap_share[POSITIONS - FINISH_BLOCK - 5] > 0.01 and gap_share[POSITIONS - FINISH_BLOCK + 5] > 0.01


@pytest.mark.parametrize("filter_index", range(4), ids=FILTERS)
@pytest.mark.parametrize("proportion", PROPORTIONS)
def test_tables_and_rows(data, filter_index, proportion):
    """The table is pre-filled with 0xFFFFFFFF: the call overwrites it."""
    (table, n_selected, rows), = scan_select(data, [filter_index], [proportion], prefill=0xFF)
    exact = data.exact[filter_index]
    want_rows = oracle_rows(exact, data.reference_index, proportion)
    assert n_selected == len(rows) == len(want_rows)
    assert rows == want_rows
    assert np.array_equal(table.sum(axis=1, dtype=np.uint32), exact.sum(axis=1, dtype=np.uint32))
    if proportion == 0:
        assert np.array_equal(table, exact)
    old_table, old_selected, old_rows = other_entries(data, filter_index, proportion)
    assert np.array_equal(table, old_table)
    assert (n_selected, rows) == (old_selected, old_rows)
    if filter_index < 2 and proportion in (0.05, 0.5):  # (the check is not vacuous: the positions with a frequent second symbol, away from the ends)
        assert {row[0] for row in rows} >= {p for p, share in FREQUENT.items() if share > 1.1 * proportion and 600 < p < 1_600}


def test_knob_off_gives_the_same_tables_and_rows(data):
    for filter_index, proportion in ((0, 0.05), (1, 0.0), (3, 0.5)):
        fused, = scan_select(data, [filter_index], [proportion], prefill=0xFF, knob=0)
        unfused, = scan_select(data, [filter_index], [proportion], prefill=0xFF, knob=-1)
        assert np.array_equal(fused[0], unfused[0])
        assert fused[1:] == unfused[1:]


def test_more_rows_than_the_slot_holds(data):
    from silo_amd import binding

    small = binding.RowSlot(4)
    try:
        (table, n_selected, rows), = scan_select(data, [0], [0.0], slots=[small], prefill=0xFF)
        want_rows = oracle_rows(data.exact[0], data.reference_index, 0.0)
        assert n_selected == len(want_rows) > 4  # the header carries the true count
        assert len(rows) == 4 and set(rows) <= set(want_rows)
        assert np.array_equal(table, data.exact[0])  # complete for the caller's fallback
    finally:
        small.close()


def test_a_slot_used_three_times_in_a_row(data):
    for filter_index, proportion in ((0, 0.05), (1, 0.5), (0, 0.0)):
        (_, n_selected, rows), = scan_select(data, [filter_index], [proportion], slots=[data.slots[0]])
        want_rows = oracle_rows(data.exact[filter_index], data.reference_index, proportion)
        assert (n_selected, rows) == (len(want_rows), want_rows)


def test_two_filters_two_tables_two_slots_in_one_call(data):
    for filter_indexes, proportions in (((0, 1), (0.05, 0.0)), ((1, 0), (0.05, 0.5))):
        results = scan_select(data, filter_indexes, proportions, prefill=0xFF)
        # (what a scan leaves out depends on all the filters of its launch: the other entry gets the same two)
        old_tables = data.store.mutations_scan_ranges([(0, 0, POSITIONS)], [data.store.filters[q] for q in filter_indexes], min_proportions=proportions)[0]
        for (table, n_selected, rows), filter_index, proportion, old_table in zip(results, filter_indexes, proportions, old_tables):
            want_rows = oracle_rows(data.exact[filter_index], data.reference_index, proportion)
            assert (n_selected, rows) == (len(want_rows), want_rows)
            assert np.array_equal(table, old_table)
            assert np.array_equal(table.sum(axis=1, dtype=np.uint32), data.exact[filter_index].sum(axis=1, dtype=np.uint32))


def test_ranges_that_do_not_tile_the_table(data):
    """Positions 10 to 300 of 2 100: the call clears the table, scans and launches the selection; the cells outside the range,
    pre-filled with 0xFFFFFFFF, are zero afterwards."""
    for proportion in (0.0, 0.05):
        (table, n_selected, rows), = scan_select(data, [0], [proportion], ranges=[(0, 10, 300)], offsets=[10], prefill=0xFF)
        old_table, old_selected, old_rows = other_entries(data, 0, proportion, [(0, 10, 300)])
        assert not table[:10].any() and not table[300:].any()
        assert np.array_equal(table, old_table)
        assert (n_selected, rows) == (old_selected, old_rows)
        reference = data.reference_index.copy()
        exact = np.zeros_like(data.exact[0])
        exact[10:300] = data.exact[0][10:300]
        assert rows == oracle_rows(exact, reference, proportion)


def test_ranges_that_tile_the_table(data):
    """Two and three ranges that tile the table: the finish kernel again, with several ranges in its launch.  The whole store has
    more one-hot rows than a scan that counts end runs lists, so its scan reads the rows of '-'; the thirds have fewer, and
    their scans count the end runs instead (", ends" in the timing log) — the same rows either way."""
    whole, = scan_select(data, [0], [0.05], prefill=0xFF)
    assert whole[2] == oracle_rows(data.exact[0], data.reference_index, 0.05)
    seen = set()
    for cuts in ((0, 1_050, POSITIONS), (0, 700, 1_400, POSITIONS), (1_400, POSITIONS, 0, 700, 1_400)):
        ranges = [(0, a, b) for a, b in zip(cuts[:-1], cuts[1:]) if a < b]
        with_ends = any(data.store.scan_rows(0, a, b) <= 1_024 for _, a, b in ranges)  # (ROW_LIST_MAX, scan_internal.h)
        seen.add(with_ends)
        kernels = []
        (table, n_selected, rows), = scan_select(data, [0], [0.05], ranges=ranges, offsets=[a for _, a, _ in ranges], prefill=0xFF, kernels=kernels)
        assert any(", ends" in k for k in kernels) == with_ends, kernels
        assert (n_selected, rows) == whole[1:]
        assert np.array_equal(table.sum(axis=1, dtype=np.uint32), data.exact[0].sum(axis=1, dtype=np.uint32))
        assert np.array_equal(table, other_entries(data, 0, 0.05, ranges)[0])
        unfused, = scan_select(data, [0], [0.05], ranges=ranges, offsets=[a for _, a, _ in ranges], prefill=0xFF, knob=-1)
        assert np.array_equal(table, unfused[0]) and (n_selected, rows) == unfused[1:]
    assert True in seen  # some scan of this test counted end runs


def test_a_store_of_identity_planes(built):
    """20 000 rows: the store keeps its build-time planes and derives nothing; the call takes the other entries' route."""
    from silo_amd import binding
    from silo_amd.binding import GpuStore

    n, positions = 20_000, 300
    rng = np.random.default_rng(97)
    sym, dominant = ragged_alignment(rng, n, positions, end_mean=30)
    mask = rng.random(n) < 0.4
    with GpuStore(n, [dict(name="main", alphabet="nuc", reference=dominant.copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_runs(0) == 0
        filter_dev = store.bitset_alloc()
        store.bitset_upload(filter_dev, dense.pack_bits(mask))
        reference = reference_index_of(store, dominant)
        reference_dev = upload_bytes(store, reference)
        slot = binding.RowSlot(CAPACITY)
        table_dev = store.malloc(4 * positions * 5)
        try:
            exact = dense.mutation_counts(sym, mask, list(store.scan_symbols[0]), 0, positions)
            for proportion in (0.0, 0.05):
                store.memset(table_dev, 0xFF, 4 * positions * 5)
                store.mutations_scan_select([(0, 0, positions)], [filter_dev], [proportion], [table_dev], [0], positions, reference_dev, [slot])
                n_selected, rows = slot.wait()
                assert np.array_equal(store.read(table_dev, np.uint32, positions * 5).reshape(positions, 5), exact)
                want_rows = oracle_rows(exact, reference, proportion)
                assert (n_selected, sorted(map(tuple, rows.tolist()))) == (len(want_rows), want_rows)
        finally:
            slot.close()
            store.lib.silo_gpu_free(reference_dev)
