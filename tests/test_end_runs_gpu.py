"""The end runs of the gap symbol in the Mutations scan: the one-hot rows of '-' at the ragged ends of an alignment are not read
but counted from one event per sequence end plus the residual keys of the rows (interior deletions, '-' cells cut off from their
run by an N).  Tables against the dense oracle, with the knob (SILO_GPU_TUNE_END_RUNS) on and off, through the exact and the
pruning entry and through the engine; the other readers still see the rows."""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
GAP, N_SYMBOL = 0, 15
AMBIGUITY_CODES = np.arange(5, 15)
TUNE_SCAN_TIMING, TUNE_LAUNCH_COST, TUNE_END_RUNS = 7, 9, 12
KEY_COST_BYTES = 10  # layout_choice.h

N, POSITIONS = 140_001, 600  # two slices of 2^17 rows, the second partial; rows long enough for k_scan_sliced
BUSY_POSITION = 40           # an end position where 30 % of the rows carry an interior deletion: its row stays uncovered
RANGES = [(0, 0, POSITIONS), (0, 10, 300), (0, 0, 30), (0, 1, 2), (0, 520, 590)]


class Built:
    pass


def ragged_alignment(rng, n, positions, lead_mean=20, trail_mean=30, second_share=0.0002):
    """One of A, C, G, T in nearly every row of a position, a second one in `second_share` of them, other symbols in 0.1 %; then
    leading and trailing runs of '-' of geometric length in 97 % of the rows."""
    dominant = rng.integers(1, 5, size=positions).astype(np.uint8)
    second = ((dominant % 4) + 1).astype(np.uint8)
    draw = rng.random((n, positions), dtype=np.float32)
    sym = np.where(draw < second_share, second, dominant).astype(np.uint8)
    lone = (draw >= second_share) & (draw < second_share + 0.001)
    sym[lone] = rng.integers(5, 16, size=int(lone.sum()))
    del draw, lone
    lead = np.where(rng.random(n) < 0.97, rng.geometric(1 / lead_mean, size=n), 0)
    trail = np.where(rng.random(n) < 0.97, rng.geometric(1 / trail_mean, size=n), 0)
    column = np.arange(positions)
    sym[column[None, :] < lead[:, None]] = GAP
    sym[column[None, :] >= positions - trail[:, None]] = GAP
    return sym, dominant, lead


def end_runs_of(sym):
    """lead[r] and trail_start[r] as the store defines them."""
    n, positions = sym.shape
    not_gap = sym != GAP
    lead = np.where(not_gap.any(axis=1), not_gap.argmax(axis=1), positions)
    last = positions - 1 - not_gap[:, ::-1].argmax(axis=1)
    trail_start = np.where(not_gap.any(axis=1), last + 1, positions)
    return lead, trail_start


def expected_end_runs(sym, row_bytes):
    """(covered rows, end events, residual keys) by the rule of the store: the row of '-' at a position that derives another
    symbol — '-' has a row there where its keys would cost more than the row — is covered where the keys of its bits outside
    the end runs cost less than the row."""
    n, positions = sym.shape
    lead, trail_start = end_runs_of(sym)
    events = int((lead < positions).sum() + (trail_start < positions).sum())
    covered = residual_keys = 0
    for p in range(positions):
        counts = np.bincount(sym[:, p], minlength=16)[:5]
        if counts.argmax() == GAP or KEY_COST_BYTES * counts[GAP] <= row_bytes:
            continue  # '-' is derived, or is kept as keys
        inside = int((lead > p).sum() + (trail_start <= p).sum())
        residual = int(counts[GAP]) - inside
        if KEY_COST_BYTES * residual < row_bytes:
            covered += 1
            residual_keys += residual
    if KEY_COST_BYTES * (events + residual_keys) >= covered * row_bytes:
        return 0, 0, 0  # the stream would cost more than the rows it replaces: the store keeps none
    return covered, events, residual_keys


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(71)
    sym, dominant, lead = ragged_alignment(rng, N, POSITIONS)
    long_lead = np.flatnonzero((lead >= 6) & (lead < POSITIONS - 20))
    for row in long_lead[:400]:  # a run of N directly behind the lead run
        sym[row, lead[row]:lead[row] + int(rng.geometric(1 / 8))] = N_SYMBOL
    for row in long_lead[400:800]:  # an N inside the lead region: the '-' cells behind it are cut off from their run
        sym[row, int(rng.integers(1, lead[row] - 1))] = N_SYMBOL
    for row in long_lead[800:1000]:  # ... and an ambiguity code
        sym[row, int(rng.integers(1, lead[row] - 1))] = rng.choice(AMBIGUITY_CODES)
    sym[rng.choice(N, size=25, replace=False)] = GAP  # '-' throughout
    sym[rng.choice(N, size=25, replace=False)] = N_SYMBOL
    ends = np.r_[0:110, POSITIONS - 150:POSITIONS]
    rare = rng.random((N, len(ends)), dtype=np.float32) < 0.0002  # rare interior deletions at end positions
    block = sym[:, ends]
    block[rare] = GAP
    sym[:, ends] = block
    sym[rng.random(N) < 0.3, BUSY_POSITION] = GAP
    one_slice = (np.arange(N) >> 17) == 1
    masks = [rng.random(N) < 0.4, rng.random(N) < 0.001, np.zeros(N, bool), np.ones(N, bool), one_slice & (rng.random(N) < 0.8),
             rng.random(N) < 0.9, (np.arange(N) >= N // 2) & (rng.random(N) < 0.7), rng.random(N) < 0.01]
    built = Built()
    built.sym, built.reference, built.masks = sym, dominant, masks
    return built


@pytest.fixture(scope="module")
def store(built, data):
    from silo_amd.binding import GpuStore

    with GpuStore(N, [dict(name="main", alphabet="nuc", reference=data.reference.copy())]) as gpu_store:
        for a in range(0, N, 35_000):
            gpu_store.append_sequences(0, a, NUC_CHARS[data.sym[a:a + 35_000]])
        gpu_store.finalize()
        assert gpu_store.scan_runs(0) > 0  # the store derives symbols and keeps N as runs
        gpu_store.filters = []
        for mask in data.masks:
            gpu_store.filters.append(gpu_store.bitset_alloc())
            gpu_store.bitset_upload(gpu_store.filters[-1], dense.pack_bits(mask))
        yield gpu_store


@pytest.fixture(scope="module")
def want(store, data):
    """The oracle's table of every filter over the whole store: computed once, sliced for the sub-ranges."""
    scan_symbols = list(store.scan_symbols[0])
    return [dense.mutation_counts(data.sym, mask, scan_symbols, 0, POSITIONS) for mask in data.masks]


def scan_with_knob(store, value, ranges, filters, **kwargs):
    """(tables[range][filter], kernel names of the timing log) with SILO_GPU_TUNE_END_RUNS = value."""
    from silo_amd import binding

    previous = store.tune(TUNE_END_RUNS, value)
    store.tune(TUNE_SCAN_TIMING, 1)
    try:
        tables = store.mutations_scan_ranges(ranges, filters, **kwargs)
        kernels = [entry["kernel"] for entry in binding.scan_timings()]
    finally:
        store.tune(TUNE_SCAN_TIMING, 0)
        store.tune(TUNE_END_RUNS, previous)
    return tables, kernels


def test_the_store_has_covered_rows_end_events_and_residual_keys(store, data):
    covered, events, residual = store.scan_end_runs(0)
    print("covered rows", covered, "end events", events, "residual keys", residual)
    assert covered > 0 and events > 0 and residual > 0
    row_bytes = 8 * (((N + 63) // 64 + 31) // 32 * 32)
    assert (covered, events, residual) == expected_end_runs(data.sym, row_bytes)
    # the busy position has a row of '-' and it is not among the covered ones: with it covered there would be one more
    busy = data.sym[:, BUSY_POSITION] == GAP
    lead, trail_start = end_runs_of(data.sym)
    assert KEY_COST_BYTES * int((busy & (lead <= BUSY_POSITION)).sum()) >= row_bytes


@pytest.mark.parametrize("q_count", [1, 2, 3, 4, 8])
def test_tables_equal_the_oracle_with_and_without_end_runs(store, data, want, q_count):
    filters = store.filters[:q_count]
    (with_ends, kernels_with), (without, kernels_without) = (scan_with_knob(store, value, RANGES, filters) for value in (0, -1))
    assert any(", ends" in k for k in kernels_with if k.startswith("k_scan_escapes_sliced<")), kernels_with
    assert any(", ends" in k for k in kernels_with if k.startswith("k_scan_sliced<2, 2,")), kernels_with
    assert not any(", ends" in k for k in kernels_without), kernels_without
    for r, (_, a, b) in enumerate(RANGES):
        for q in range(q_count):
            assert np.array_equal(with_ends[r][q], want[q][a:b]), (a, b, q)
            assert np.array_equal(without[r][q], want[q][a:b]), (a, b, q)


def test_end_events_in_a_launch_of_their_own(store, data, want):
    """SILO_GPU_TUNE_END_RUNS = 1 (kept for comparisons): the end events and the residual keys in a second launch of the escape
    kernel behind the row launch; the same tables."""
    tables, kernels = scan_with_knob(store, 1, RANGES, store.filters[:2])
    escapes = [k for k in kernels if k.startswith("k_scan_escapes_sliced<")]
    assert len(escapes) == 2 and ", ends" not in escapes[0] and ", ends" in escapes[1], kernels
    for r, (_, a, b) in enumerate(RANGES):
        for q in range(2):
            assert np.array_equal(tables[r][q], want[q][a:b]), (a, b, q)


# ---- the pruning entry: the rule and the helpers of tests/test_pruned_scan_gpu.py -------------------------------------------------
def must_exceed(covered, proportion):
    return int(math.ceil(float(covered) * proportion) - 1)


def reference_index(store, data, a=0, b=POSITIONS):
    scan_symbols = list(store.scan_symbols[0])
    return np.array([scan_symbols.index(s) if s in scan_symbols else 255 for s in data.reference[a:b]], dtype=np.uint8)


def selected_rows(store, table, reference, proportion):
    n, rows = store.mutations_select(table, reference, proportion, capacity=table.size)
    assert n == len(rows)
    return sorted(map(tuple, rows.tolist()))


def check_against_exact(store, data, pruned, exact, proportion, a=0, b=POSITIONS, label=""):
    assert np.array_equal(pruned.sum(axis=1), exact.sum(axis=1)), (label, proportion)
    reference = reference_index(store, data, a, b)
    assert selected_rows(store, pruned, reference, proportion) == selected_rows(store, exact, reference, proportion), (label, proportion)


def test_pruning_entry_selects_the_rows_of_the_exact_scan(store, data, want):
    """Eight filters, each with its own proportion, over the whole store and two sub-ranges; with the knob on and off."""
    proportions = [0.05, 0.01, 0.5, 0.01, 0.05, 0.5, 0.01, 0.05]
    ranges = [RANGES[0], RANGES[1], RANGES[4]]
    for value in (0, -1):
        tables, kernels = scan_with_knob(store, value, ranges, store.filters, min_proportions=proportions)
        assert any(", pruning" in k for k in kernels), kernels
        assert any(", ends" in k for k in kernels) == (value == 0), kernels
        for (_, a, b), per_filter in zip(ranges, tables):
            for q, (proportion, pruned) in enumerate(zip(proportions, per_filter)):
                check_against_exact(store, data, pruned, want[q][a:b], proportion, a, b, label=(value, q, a, b))
    for proportion in (0.01, 0.05, 0.5):  # one filter per call
        pruned = store.mutations_scan_ranges([RANGES[0]], [store.filters[0]], min_proportions=[proportion])[0][0]
        check_against_exact(store, data, pruned, want[0], proportion, label="one filter")


def test_a_range_of_more_rows_than_the_list_holds_reads_its_rows(built):
    """Every position with a second symbol in 5 % of the rows, so a one-hot row each, plus the rows of '-' at the ragged ends: more
    than ROW_LIST_MAX rows in the one run.  The whole range reads its rows and counts no end events; a sub-range of fewer rows
    counts them."""
    from silo_amd.binding import GpuStore

    n, positions = 70_001, 1_200
    rng = np.random.default_rng(73)
    sym, dominant, _ = ragged_alignment(rng, n, positions, second_share=0.05)
    masks = [rng.random(n) < 0.4, np.ones(n, bool)]
    with GpuStore(n, [dict(name="main", alphabet="nuc", reference=dominant.copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_end_runs(0)[0] > 0
        assert store.scan_rows(0, 0, positions) > 1024
        filters = []
        for mask in masks:
            filters.append(store.bitset_alloc())
            store.bitset_upload(filters[-1], dense.pack_bits(mask))
        scan_symbols = list(store.scan_symbols[0])
        for (a, b), ends in (((0, positions), False), ((0, 200), True)):
            assert (store.scan_rows(0, a, b) <= 1024) == ends
            tables, kernels = scan_with_knob(store, 0, [(0, a, b)], filters)
            assert any(", ends" in k for k in kernels) == ends, kernels
            for q, mask in enumerate(masks):
                assert np.array_equal(tables[0][q], dense.mutation_counts(sym, mask, scan_symbols, a, b)), (a, b, q)


def test_a_store_without_the_end_stream(built):
    """1 000 rows: the store keeps its build-time planes (the row-wave kernel), has no end runs and scans right."""
    from silo_amd import binding
    from silo_amd.binding import GpuStore

    n, positions = 1_000, 200
    rng = np.random.default_rng(79)
    sym, dominant, _ = ragged_alignment(rng, n, positions)
    mask = rng.random(n) < 0.5
    with GpuStore(n, [dict(name="main", alphabet="nuc", reference=dominant.copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_end_runs(0) == (0, 0, 0)
        ptr = store.bitset_alloc()
        store.bitset_upload(ptr, dense.pack_bits(mask))
        assert np.array_equal(store.mutations_scan(0, ptr), dense.mutation_counts(sym, mask, list(store.scan_symbols[0])))
        assert binding.load_library().silo_gpu_last_scan_kernel().decode() == "k_scan_sliced_rowwave"


# ---- through the engine ------------------------------------------------------------------------------------------------------------
PART_ROWS = 66_000  # a partition's stores are re-encoded from 65 536 rows on
COVERED_POSITION = 30  # '-' in about a fifth of the rows of "main": a one-hot row, covered


def engine_of(n_partitions):
    from silo_amd.engine import Engine

    rng = np.random.default_rng(83)
    rows = PART_ROWS * n_partitions
    bucket = rng.integers(0, 10, size=rows)
    references, sequences, chars_of = {}, {}, {}
    for name, is_aa, positions, letters, missing in (("main", False, 300, "ACGT", "N"), ("S", True, 120, "ACDEFGHIKLMNPQRSTVWY", "X")):
        alphabet = np.frombuffer(letters.encode(), dtype=np.uint8)
        reference_index = rng.integers(0, len(alphabet), size=positions)
        reference = alphabet[reference_index]
        second = alphabet[(reference_index + 1) % len(alphabet)]
        draw = rng.random((rows, positions), dtype=np.float32)
        chars = np.where(draw < 0.002, second, reference).astype(np.uint8)
        for p in (positions // 3, positions // 2):  # reported at 0.05
            chars[rng.random(rows) < 0.08, p] = second[p]
        lead = np.where(rng.random(rows) < 0.97, rng.geometric(1 / 20, size=rows), 0)
        trail = np.where(rng.random(rows) < 0.97, rng.geometric(1 / 40, size=rows), 0)
        column = np.arange(positions)
        chars[column[None, :] < lead[:, None]] = ord("-")
        chars[column[None, :] >= positions - trail[:, None]] = ord("-")
        for row in rng.choice(rows, size=300 * n_partitions, replace=False):  # runs of the missing symbol, some inside the lead region
            start = int(rng.integers(0, positions))
            chars[row, start:start + int(rng.geometric(1 / 20))] = ord(missing)
        interior = rng.random((rows, 60), dtype=np.float32) < 0.0005  # interior deletions at the front
        block = chars[:, :60]
        block[interior] = ord("-")
        chars[:, :60] = block
        references[name] = bytes(reference).decode()
        sequences[name] = [bytes(row).decode() for row in chars]
        chars_of[name] = chars
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": references["main"]}], "genes": [{"name": "S", "sequence": references["S"]}]})
    engine.set_schema("key", "date")
    for k in range(n_partitions):
        lo, hi = k * PART_ROWS, (k + 1) * PART_ROWS
        part = engine.add_partition(PART_ROWS)
        for name, is_aa in (("main", False), ("S", True)):
            engine.append_sequences(part, name, is_aa, 0, sequences[name][lo:hi])
        engine.append_metadata(part, "key", "string", [str(i) for i in range(lo, hi)])
        engine.append_metadata(part, "date", "date", ["2021-03-04"] * PART_ROWS)
        engine.append_metadata(part, "bucket", "int", [str(b) for b in bucket[lo:hi]])
    engine.finalize()
    return engine, chars_of


@pytest.mark.parametrize("n_partitions", [1, 2])
def test_engine_bodies_do_not_depend_on_the_knob(built, n_partitions):
    from silo_amd import binding

    lib = binding.load_library()
    lib.silo_gpu_tune(TUNE_LAUNCH_COST, -1)
    try:
        engine, chars_of = engine_of(n_partitions)
    finally:
        lib.silo_gpu_tune(TUNE_LAUNCH_COST, 0)
    for k in range(n_partitions):
        view = engine.partition_store(k)
        assert int(lib.silo_gpu_store_scan_covered_rows(view.handle, engine.seqstore_id(k, "main", False))) > 0, k
    queries = [json.dumps({"action": {"type": action, "minProportion": 0.05}, "filterExpression": {"type": "IntBetween", "column": "bucket", "from": 0, "to": 3}})
               for action in ("Mutations", "AminoAcidMutations")]
    bodies, ends = {}, {}
    for value in (0, -1):
        previous = lib.silo_gpu_tune(TUNE_END_RUNS, value)
        lib.silo_gpu_tune(TUNE_SCAN_TIMING, 1)
        try:
            bodies[value], ends[value] = [], []
            for query in queries:
                bodies[value].append(engine.execute_text(query))
                ends[value].append(any(", ends" in entry["kernel"] for entry in binding.scan_timings()))  # (the query's last scan)
        finally:
            lib.silo_gpu_tune(TUNE_SCAN_TIMING, 0)
            lib.silo_gpu_tune(TUNE_END_RUNS, previous)
    assert all(status == 200 for status, _ in bodies[0]), bodies[0]
    assert bodies[0] == bodies[-1]
    assert ends[0][0] and ends[-1] == [False, False]
    assert all(json.loads(body)["queryResult"] for _, body in bodies[0])
    # the other readers still see the row: a filter leaf on '-' at a covered position
    status, body = engine.execute_text(json.dumps({
        "action": {"type": "Aggregated"}, "filterExpression": {"type": "NucleotideEquals", "position": COVERED_POSITION + 1, "symbol": "-"}}))
    assert status == 200
    assert json.loads(body)["queryResult"][0]["count"] == int((chars_of["main"][:, COVERED_POSITION] == ord("-")).sum())
