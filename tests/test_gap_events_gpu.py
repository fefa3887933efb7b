"""The gap events of a store with derived symbols: the rows without a valid symbol at a position (runs of N, ambiguity codes)
counted by the escape pass from the store's slice-major gap events, against the direct count and against the runs and sparse
keys counted by themselves (SILO_GPU_TUNE_GAP_EVENTS < 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
N_SYMBOL = 15
AMBIGUITY_CODES = np.arange(5, 15)
TUNE_SCAN_TIMING, TUNE_LAUNCH_COST, TUNE_GAP_EVENTS = 7, 9, 10


def settled_alignment(rng, n, positions):
    """Per position one valid symbol in nearly every row, a second one in 0.02 %, the rest of the valid symbols 0.01 % and
    the other symbols 0.1 %: positions that derive their most numerous symbol."""
    from silo_amd import alphabet as alphabets

    table = alphabets.NUCLEOTIDE
    valid = np.array(list(table.valid_mutation_symbols))
    others = np.array([s for s in range(table.count) if s not in set(valid.tolist())])
    sym = np.empty((n, positions), dtype=np.uint8)
    for p in range(positions):
        order = rng.permutation(valid)
        probs = np.zeros(table.count)
        probs[order[0]], probs[order[1]] = 0.9987, 0.0002
        probs[order[2:]] = 0.0001 / (len(valid) - 2)
        probs[others] = 0.001 / len(others)
        sym[:, p] = rng.choice(table.count, size=n, p=probs / probs.sum())
    return sym


def add_gaps(rng, sym, rows_with_runs):
    """Runs of N (geometric lengths, mean ~300) in some rows, some from position 0, a few rows N throughout, ambiguity codes
    next to runs and on their own."""
    n, positions = sym.shape
    rows = rng.choice(n, size=rows_with_runs, replace=False)
    for k, row in enumerate(rows):
        for _ in range(1 + k % 3):
            start = 0 if k % 7 == 0 else int(rng.integers(0, positions))
            end = min(positions, start + int(rng.geometric(1 / 300)))
            sym[row, start:end] = N_SYMBOL
            if k % 5 == 0 and end < positions:
                sym[row, end] = rng.choice(AMBIGUITY_CODES)  # a code right behind the run
            if k % 5 == 1 and start > 0:
                sym[row, start - 1] = rng.choice(AMBIGUITY_CODES)  # and right in front of it
    sym[rng.choice(n, size=max(1, n // 1000), replace=False)] = N_SYMBOL  # rows missing throughout
    lone = rng.random(sym.shape) < 0.0005
    sym[lone] = rng.choice(AMBIGUITY_CODES, size=int(lone.sum()))


def make_store(n, sym):
    from silo_amd.binding import GpuStore

    return GpuStore(n, [dict(name="main", alphabet="nuc", reference=sym[0].copy())])


def scan_both_ways(store, ranges, filters):
    """tables[range][filter] with the gap events and with the runs and sparse keys by themselves; the launches of each."""
    from silo_amd import binding

    out = []
    for value in (0, -1):
        previous = store.tune(TUNE_GAP_EVENTS, value)
        store.tune(TUNE_SCAN_TIMING, 1)
        try:
            tables = store.mutations_scan_ranges(ranges, filters)
            kernels = [e["kernel"] for e in binding.scan_timings()]
        finally:
            store.tune(TUNE_SCAN_TIMING, 0)
            store.tune(TUNE_GAP_EVENTS, previous)
        out.append((tables, kernels))
    return out


def upload(store, masks):
    pointers = []
    for mask in masks:
        ptr = store.bitset_alloc()
        store.bitset_upload(ptr, dense.pack_bits(mask))
        pointers.append(ptr)
    return pointers


def check(store, sym, ranges, masks, filters):
    scan_symbols = list(store.scan_symbols[0])
    (events, event_kernels), (separate, separate_kernels) = scan_both_ways(store, ranges, filters)
    assert not any(k.startswith(("k_scan_missing_runs", "k_count_sparse_keys")) for k in event_kernels), event_kernels
    assert any(k.startswith("k_scan_missing_runs") for k in separate_kernels), separate_kernels
    for r, (_, a, b) in enumerate(ranges):
        for q, mask in enumerate(masks):
            want = dense.mutation_counts(sym, mask, scan_symbols, a, b)
            assert np.array_equal(events[r][q], want), (a, b, q)
            assert np.array_equal(separate[r][q], want), (a, b, q)


def test_gap_events_over_filters_and_sub_ranges(built):
    """Three slices of rows, the last partial; 1, 2, 3, 4 and 8 filters in one call over the whole store and over sub-ranges
    whose first and last positions lie inside runs; filters that are empty, full, or empty over a whole slice."""
    rng = np.random.default_rng(41)
    n, positions = 300001, 700
    sym = settled_alignment(rng, n, positions)
    add_gaps(rng, sym, 9000)
    no_middle_slice = (rng.random(n) < 0.5) & ((np.arange(n) >> 17) != 1)
    masks = [rng.random(n) < 0.4, no_middle_slice, np.zeros(n, bool), np.ones(n, bool),
             rng.random(n) < 0.01, (np.arange(n) >= n // 2) & (rng.random(n) < 0.7), rng.random(n) < 0.9, rng.random(n) < 0.2]
    # sub-ranges that begin and end inside the runs of many rows
    ranges = [(0, 0, positions), (0, 123, 456), (0, 1, 2), (0, 300, positions), (0, 650, 699)]
    with make_store(n, sym) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_runs(0) > 0  # the store derives symbols and keeps N as runs
        filters = upload(store, masks)
        for q_count in (1, 2, 3, 4, 8):
            check(store, sym, ranges, masks[:q_count], filters[:q_count])


def test_gap_events_of_a_small_sparse_store(built):
    """One slice of rows and gap events thousands of positions apart: a granule of gap events ends early (events have no
    overflow list)."""
    rng = np.random.default_rng(43)
    n, positions = 65600, 6500  # (the fewest rows whose store is re-encoded, not kept as identity planes)
    sym = np.tile(rng.integers(1, 5, size=positions).astype(np.uint8), (n, 1))
    for p in range(0, positions, 97):  # a few valid mutations
        sym[rng.choice(n, size=3, replace=False), p] = (sym[0, p] % 4) + 1
    sym[5, 10:30] = N_SYMBOL
    sym[6, 0:3] = N_SYMBOL
    sym[7, 3200:3250] = N_SYMBOL
    sym[8, 3240] = AMBIGUITY_CODES[2]
    sym[10, 3300] = AMBIGUITY_CODES[0]
    sym[10, 3301:3310] = N_SYMBOL
    sym[9, 6400:] = N_SYMBOL
    masks = [rng.random(n) < 0.5, np.ones(n, bool)]
    ranges = [(0, 0, positions), (0, 20, 3245), (0, 3305, 6450)]
    with make_store(n, sym) as store:
        store.tune(TUNE_LAUNCH_COST, -1)  # (no charge per kind of launch: a small store is to derive symbols too)
        try:
            for a in range(0, n, 16400):
                store.append_sequences(0, a, NUC_CHARS[sym[a:a + 16400]])
            store.finalize()
        finally:
            store.tune(TUNE_LAUNCH_COST, 0)
        assert store.scan_runs(0) > 0
        filters = upload(store, masks)
        for q_count in (1, 2):
            check(store, sym, ranges, masks[:q_count], filters[:q_count])


def test_two_pass_store_gives_the_same_gap_tables(built):
    """A store built in two passes (counted, then encoded straight into the adaptive planes) has the same gap events."""
    rng = np.random.default_rng(47)
    n, positions = 140000, 400
    sym = settled_alignment(rng, n, positions)
    add_gaps(rng, sym, 3000)
    cuts = [0, n // 3 + 17, 2 * n // 3 + 5, n]
    masks = [rng.random(n) < 0.4, np.ones(n, bool)]
    ranges = [(0, 0, positions), (0, 77, 333)]
    results = []
    for two_pass in (False, True):
        with make_store(n, sym) as store:
            if two_pass:
                store.build_pass(0, 1)
                for a, b in zip(cuts[:-1], cuts[1:]):
                    store.append_sequences(0, a, NUC_CHARS[sym[a:b]])
                store.build_pass(0, 2)
            for a, b in zip(cuts[:-1], cuts[1:]):
                store.append_sequences(0, a, NUC_CHARS[sym[a:b]])
            store.finalize()
            assert store.scan_runs(0) > 0
            filters = upload(store, masks)
            check(store, sym, ranges, masks, filters)
            results.append(store.mutations_scan_ranges(ranges, filters))
    tables_one, tables_two = results
    for r in range(len(ranges)):
        for q in range(len(masks)):
            assert np.array_equal(tables_one[r][q], tables_two[r][q])
