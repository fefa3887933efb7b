"""The escape pass on blocks that walk the launch's items — (range, slice, share) — in turn (k_scan_escapes_sliced,
SILO_GPU_TUNE_ESCAPE_BLOCKS): the same tables whatever the number of blocks, byte for byte those of one block per item; against
the dense oracle, through the exact and the pruning entry, for one, two and eight filters per pass, in one launch over several
ranges and over two stores.  Two slices, the second partial; every launch has more items than the 1, 2, 3 or 5 blocks it is given."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
GAP, N_SYMBOL = 0, 15
AMBIGUITY_CODES = np.arange(5, 15)
TUNE_SCAN_TIMING, TUNE_ESCAPE_BLOCKS = 7, 14
KNOBS = (0, -1, 1, 2, 3, 5)  # one block per item (the default and the reference), resident blocks, exactly n blocks planned as for n places

N, POSITIONS = 140_001, 600  # two slices of 2^17 rows, the second partial
SECOND_POSITIONS = 250       # the second store of the two-store database
RANGES = [(0, 0, POSITIONS), (0, 10, 300), (0, 1, 2), (0, 520, 590)]  # the whole store; beginning inside runs; one position; the far end
PROPORTIONS = (0.0, 0.05, 0.5)
FILTER_NAMES = ["random 40 %", "a few hundred rows", "empty", "second slice only", "all rows"]
BATCHES = {  # filters per call: the instantiations <1>, <2> and <8>
    1: [[name] for name in FILTER_NAMES],
    2: [["random 40 %", "second slice only"], ["a few hundred rows", "empty"], ["all rows", "random 40 %"]],
    # (with the empty filter, or the few hundred rows, in the pass no granule can be skipped: the second batch is without them)
    8: [FILTER_NAMES + ["second slice only", "random 40 %", "all rows"],
        ["random 40 %", "all rows", "second slice only", "random 40 %", "all rows", "second slice only", "all rows", "random 40 %"]],
}


class Built:
    pass


def alignment(rng, n, positions):
    """Settled positions (one of A, C, G, T in nearly every row, a second one in 0.2 %: keys), other symbols in 0.1 %, leading and
    trailing runs of '-' of geometric length in 97 % of the rows (end events), runs of N — some from position 0, some rows missing
    throughout — (gap events), rare interior deletions at the end positions (residual keys)."""
    dominant = rng.integers(1, 5, size=positions).astype(np.uint8)
    second = ((dominant % 4) + 1).astype(np.uint8)
    draw = rng.random((n, positions), dtype=np.float32)
    sym = np.where(draw < 0.002, second, dominant).astype(np.uint8)
    lone = (draw >= 0.002) & (draw < 0.003)
    sym[lone] = rng.integers(5, 16, size=int(lone.sum()))
    del draw, lone
    for p in (150, 400):  # a substitution that is reported at 0.05
        sym[rng.random(n) < 0.08, p] = second[p]
    lead = np.where(rng.random(n) < 0.97, rng.geometric(1 / 20, size=n), 0)
    trail = np.where(rng.random(n) < 0.97, rng.geometric(1 / 30, size=n), 0)
    column = np.arange(positions)
    sym[column[None, :] < lead[:, None]] = GAP
    sym[column[None, :] >= positions - trail[:, None]] = GAP
    for k, row in enumerate(rng.choice(n, size=1500, replace=False)):  # runs of N, ambiguity codes beside some
        start = 0 if k % 7 == 0 else int(rng.integers(0, positions))
        end = min(positions, start + int(rng.geometric(1 / 150)))
        sym[row, start:end] = N_SYMBOL
        if k % 5 == 0 and end < positions:
            sym[row, end] = rng.choice(AMBIGUITY_CODES)
    sym[rng.choice(n, size=25, replace=False)] = GAP  # '-' throughout
    sym[rng.choice(n, size=n // 1000, replace=False)] = N_SYMBOL  # rows missing throughout
    ends = np.r_[0:110, positions - 150:positions]
    rare = rng.random((n, len(ends)), dtype=np.float32) < 0.0002  # interior deletions at end positions
    block = sym[:, ends]
    block[rare] = GAP
    sym[:, ends] = block
    return sym, dominant


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(101)
    built = Built()
    built.sym, built.reference = alignment(rng, N, POSITIONS)
    # the second store: the far end of the first, turned round (its trailing runs lead)
    built.sym_second = np.ascontiguousarray(built.sym[:, ::-1][:, :SECOND_POSITIONS])
    built.reference_second = np.ascontiguousarray(built.reference[::-1][:SECOND_POSITIONS])
    one_slice = (np.arange(N) >> 17) == 1
    built.masks = {
        "random 40 %": rng.random(N) < 0.4,
        "a few hundred rows": rng.random(N) < 0.002,
        "empty": np.zeros(N, bool),
        "second slice only": one_slice & (rng.random(N) < 0.8),  # items of the first slice leave without a selected row, between counted ones
        "all rows": np.ones(N, bool),
    }
    return built


@pytest.fixture(scope="module")
def store(built, data):
    from silo_amd.binding import GpuStore

    stores = [dict(name="main", alphabet="nuc", reference=data.reference.copy()), dict(name="second", alphabet="nuc", reference=data.reference_second.copy())]
    with GpuStore(N, stores) as gpu_store:
        for a in range(0, N, 35_000):
            gpu_store.append_sequences(0, a, NUC_CHARS[data.sym[a:a + 35_000]])
            gpu_store.append_sequences(1, a, NUC_CHARS[data.sym_second[a:a + 35_000]])
        gpu_store.finalize()
        gpu_store.filters = {}
        for name, mask in data.masks.items():
            gpu_store.filters[name] = gpu_store.bitset_alloc()
            gpu_store.bitset_upload(gpu_store.filters[name], dense.pack_bits(mask))
        yield gpu_store


@pytest.fixture(scope="module")
def want(store, data):
    """The oracle's table of every filter over the whole of both stores: computed once, sliced for the sub-ranges."""
    tables = {}
    for seqstore_id, sym, positions in ((0, data.sym, POSITIONS), (1, data.sym_second, SECOND_POSITIONS)):
        scan_symbols = list(store.scan_symbols[seqstore_id])
        tables[seqstore_id] = {name: dense.mutation_counts(sym, mask, scan_symbols, 0, positions) for name, mask in data.masks.items()}
    return tables


def scan_with_blocks(store, knob, ranges, names, min_proportions=None):
    """(tables[range][filter], the escape launches of the timing log, the item count of the last one) with SILO_GPU_TUNE_ESCAPE_BLOCKS = knob."""
    from silo_amd import binding

    previous = store.tune(TUNE_ESCAPE_BLOCKS, knob)
    store.tune(TUNE_SCAN_TIMING, 1)
    try:
        tables = store.mutations_scan_ranges(ranges, [store.filters[name] for name in names], min_proportions=min_proportions)
        launches = [entry for entry in binding.scan_timings() if entry["kernel"].startswith("k_scan_escapes_sliced<")]
        items = int(binding.load_library().silo_gpu_last_escape_items())
    finally:
        store.tune(TUNE_SCAN_TIMING, 0)
        store.tune(TUNE_ESCAPE_BLOCKS, previous)
    return tables, launches, items


def reference_index(store, reference, seqstore_id, a, b):
    scan_symbols = list(store.scan_symbols[seqstore_id])
    return np.array([scan_symbols.index(s) if s in scan_symbols else 255 for s in reference[a:b]], dtype=np.uint8)


def selected_rows(store, table, reference, proportion):
    n, rows = store.mutations_select(table, reference, proportion, capacity=table.size)
    assert n == len(rows)
    return sorted(map(tuple, rows.tolist()))


def check_against_exact(store, reference, pruned, exact, proportion, label):
    """The rule of tests/test_pruned_scan_gpu.py: every position's row sum and the selected rows are those of the exact table."""
    assert np.array_equal(pruned.sum(axis=1), exact.sum(axis=1)), label
    assert selected_rows(store, pruned, reference, proportion) == selected_rows(store, exact, reference, proportion), label


def check_blocks(knob, launches, items, passes=1):
    """The grid the timing log reports against the knob and the item count of the accessor."""
    assert launches and items > 0, (knob, launches)
    blocks = launches[-1]["blocks"]
    assert blocks % passes == 0
    if knob == 0:
        assert blocks == items * passes, (knob, blocks, items)
    elif knob > 0:
        assert blocks == min(knob, items) * passes, (knob, blocks, items)
    else:
        assert 1 <= blocks <= items * passes, (knob, blocks, items)


def test_the_store_has_all_four_kinds_of_entries_and_enough_items(store):
    """What the other tests stand on: keys, gap events, end events and residual keys, and a launch over the whole store of at least
    8 items — more than the 5 blocks of the largest grid below — in at least two entries and both slices."""
    for seqstore_id in (0, 1):
        assert store.scan_runs(seqstore_id) > 0  # the store derives symbols and keeps N as runs: gap events
        assert int(store.scan_escapes(seqstore_id)) > 0
    covered, events, residual = store.scan_end_runs(0)
    print("covered rows", covered, "end events", events, "residual keys", residual, "escape keys", int(store.scan_escapes(0)))
    assert covered > 0 and events > 0 and residual > 0
    _, launches, items = scan_with_blocks(store, 0, [RANGES[0]], ["random 40 %"])
    assert len(launches) == 1 and ", ends" in launches[0]["kernel"], launches
    assert items >= 8 and items % 2 == 0 and items // 2 >= 4, items  # (every entry has the same number of items in both slices; four entries)
    _, launches, pruned_items = scan_with_blocks(store, 0, [RANGES[0]], ["random 40 %"], min_proportions=[0.05])
    assert ", pruning" in launches[0]["kernel"] and pruned_items >= 8, (launches, pruned_items)


def test_one_block_walks_every_item(store, data, want):
    """SILO_GPU_TUNE_ESCAPE_BLOCKS = 1: a single block takes every item of the launch, entry after entry, slice after slice."""
    for min_proportions in (None, [0.05]):
        tables, launches, items = scan_with_blocks(store, 1, [RANGES[0]], ["random 40 %"], min_proportions=min_proportions)
        assert len(launches) == 1 and launches[0]["blocks"] == 1 and items >= 8, (launches, items)
        if min_proportions is None:
            assert np.array_equal(tables[0][0], want[0]["random 40 %"])


@pytest.mark.parametrize("per_pass", sorted(BATCHES))
def test_tables_do_not_depend_on_the_blocks(store, data, want, per_pass):
    """Exact entry and pruning entry at 0, 0.05 and 0.5 over four ranges in one call: under every knob value byte for byte the tables
    of one block per item; those equal the oracle (exact entry, and a proportion of 0) or select the oracle's rows (pruning entry)."""
    skipped = False
    for names in BATCHES[per_pass]:
        for proportion in (None, *PROPORTIONS):
            min_proportions = None if proportion is None else [proportion] * len(names)
            tables = {}
            for knob in KNOBS:
                tables[knob], launches, items = scan_with_blocks(store, knob, RANGES, names, min_proportions=min_proportions)
                assert all(entry["kernel"].startswith(f"k_scan_escapes_sliced<{per_pass}>") for entry in launches), launches
                if proportion:
                    assert any(", pruning" in entry["kernel"] for entry in launches), (launches, proportion)
                check_blocks(knob, launches, items)
                if knob > 0:
                    assert items > knob, (items, knob)  # more items than blocks: every block walks several
            for r, (_, a, b) in enumerate(RANGES):
                for q, name in enumerate(names):
                    reference_table = tables[0][r][q]
                    for knob in KNOBS[1:]:
                        assert tables[knob][r][q].tobytes() == reference_table.tobytes(), (knob, names, name, proportion, a, b)
                    exact = want[0][name][a:b]
                    if not proportion:
                        assert np.array_equal(reference_table, exact), (names, name, proportion, a, b)
                    else:
                        check_against_exact(store, reference_index(store, data.reference, 0, a, b), reference_table, exact, proportion, (names, name, proportion, a, b))
                        skipped = skipped or not np.array_equal(reference_table, exact)
    assert skipped  # (the pruning entry did leave granules out: its exits were taken)


@pytest.mark.parametrize("per_pass", [1, 8])
def test_two_stores_in_one_call(store, data, want, per_pass):
    """Ranges of both sequence stores of the database in one silo_gpu_mutations_scan_ranges call: the multi-range launch of the
    amino-acid query."""
    ranges = [(0, 0, POSITIONS), (1, 0, SECOND_POSITIONS), (1, 7, 130), (0, 10, 300)]
    names = BATCHES[per_pass][1] if per_pass == 8 else ["random 40 %"]
    references = {0: data.reference, 1: data.reference_second}
    for proportion in (None, 0.05):
        min_proportions = None if proportion is None else [proportion] * len(names)
        tables = {}
        for knob in KNOBS:
            tables[knob], launches, items = scan_with_blocks(store, knob, ranges, names, min_proportions=min_proportions)
            check_blocks(knob, launches, items)
        for r, (seqstore_id, a, b) in enumerate(ranges):
            for q, name in enumerate(names):
                reference_table = tables[0][r][q]
                for knob in KNOBS[1:]:
                    assert tables[knob][r][q].tobytes() == reference_table.tobytes(), (knob, name, proportion, seqstore_id, a, b)
                exact = want[seqstore_id][name][a:b]
                if proportion is None:
                    assert np.array_equal(reference_table, exact), (name, seqstore_id, a, b)
                else:
                    check_against_exact(store, reference_index(store, references[seqstore_id], seqstore_id, a, b), reference_table, exact, proportion,
                                        (name, proportion, seqstore_id, a, b))
