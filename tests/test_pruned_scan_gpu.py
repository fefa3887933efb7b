"""The Mutations scan that may leave out escape keys below a filter's minProportion
(silo_gpu_mutations_scan_ranges_min_proportion): the rows silo_gpu_mutations_select reports, and every position's row sum, against
the exact entry and against the dense oracle."""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
N_SYMBOL = 15
AMBIGUITY_CODES = np.arange(5, 15)
TUNE_LAUNCH_COST, TUNE_PRUNE_KEYS = 9, 11
PROPORTIONS = (0.0, 0.01, 0.05, 0.5, 1.0)

N, POSITIONS = 140_000, 600  # two slices of 2^17 rows, the second partial; not a multiple of 2048 rows
# crafted positions, a granule of keys (~15 positions in the first slice) or more apart
AT_BOUND, ABOVE_BOUND = 100, 300          # under the all-rows filter at 0.01: a group of exactly must_exceed keys, and of one more
F_AT_BOUND, F_ABOVE_BOUND = 200, 250      # under the 40 % filter at 0.05, all their rows inside the filter
OTHER_REFERENCE = 450                     # the most numerous symbol is not the reference symbol
CODE_PLANES = range(500, 512)             # four symbols a quarter of the rows each: two code planes, nothing derived
AMBIGUOUS_AT_CRAFTED = 6000               # rows with an ambiguity code at AT_BOUND / ABOVE_BOUND: more than anywhere around them


def must_exceed(covered, proportion):
    return int(math.ceil(float(covered) * proportion) - 1)


class Built:
    pass


@pytest.fixture(scope="module")
def data():
    """Settled positions (one symbol in nearly every row, a second one in 0.2 %: ~43 granules of keys), geometric runs of N,
    ambiguity codes, and the crafted positions."""
    rng = np.random.default_rng(53)
    valid = np.array([0, 1, 2, 3, 4])
    orders = np.array([rng.permutation(valid) for _ in range(POSITIONS)], dtype=np.uint8)
    dominant, second = orders[:, 0].copy(), orders[:, 1].copy()
    draw = rng.random((N, POSITIONS), dtype=np.float32)
    sym = np.where(draw < 0.002, second, dominant).astype(np.uint8)          # the second symbol in 0.2 % of the rows
    sym = np.where((draw >= 0.002) & (draw < 0.0022), orders[:, 2], sym)     # a third one in 0.02 %
    lone = (draw >= 0.0022) & (draw < 0.0032)                                # other symbols in 0.1 %
    sym[lone] = rng.integers(5, 16, size=int(lone.sum()))
    del draw
    rows = rng.choice(N, size=1500, replace=False)
    for k, row in enumerate(rows):  # runs of N, some from position 0, ambiguity codes beside them
        for _ in range(1 + k % 3):
            start = 0 if k % 7 == 0 else int(rng.integers(0, POSITIONS))
            end = min(POSITIONS, start + int(rng.geometric(1 / 150)))
            sym[row, start:end] = N_SYMBOL
            if k % 5 == 0 and end < POSITIONS:
                sym[row, end] = rng.choice(AMBIGUITY_CODES)
    sym[rng.choice(N, size=N // 1000, replace=False)] = N_SYMBOL  # rows missing throughout
    mask40 = rng.random(N) < 0.4

    def craft(position, group_rows, ambiguous_rows):
        sym[:, position] = dominant[position]
        sym[ambiguous_rows, position] = AMBIGUITY_CODES[position % len(AMBIGUITY_CODES)]
        sym[group_rows, position] = second[position]

    # all rows at 0.01: covered = N - 6000 at both positions, the largest number of rows without a symbol of their granules
    bound_all = must_exceed(N - AMBIGUOUS_AT_CRAFTED, 0.01)
    for position, total in ((AT_BOUND, bound_all), (ABOVE_BOUND, bound_all + 1)):
        chosen = rng.permutation(N)
        craft(position, chosen[:total], chosen[total:total + AMBIGUOUS_AT_CRAFTED])
    # the 40 % filter at 0.05: every row has a valid symbol there, covered = |filter|
    bound_40 = must_exceed(int(mask40.sum()), 0.05)
    inside = np.flatnonzero(mask40)
    for position, total in ((F_AT_BOUND, bound_40), (F_ABOVE_BOUND, bound_40 + 1)):
        craft(position, rng.permutation(inside)[:total], np.zeros(0, dtype=np.int64))
    for position in CODE_PLANES:  # four symbols a quarter each, the fifth in ~100 rows: keys of a position that derives nothing
        order = rng.permutation(valid)
        sym[:, position] = order[rng.integers(0, 4, size=N)]
        sym[rng.choice(N, size=100, replace=False), position] = order[4]
    reference = dominant.copy()
    reference[OTHER_REFERENCE] = second[OTHER_REFERENCE]
    one_slice = (np.arange(N) >> 17) == 1
    masks = {
        "random 40 %": mask40,
        "a few hundred rows": rng.random(N) < 0.002,
        "empty": np.zeros(N, bool),
        "second slice only": one_slice & (rng.random(N) < 0.8),
        "all rows": np.ones(N, bool),  # (pack_bits leaves the padding bits beyond sequence_count clear)
    }
    built = Built()
    built.sym, built.reference, built.masks, built.bound_all, built.bound_40 = sym, reference, masks, bound_all, bound_40
    built.second = second
    return built


@pytest.fixture(scope="module")
def store(built, data):
    from silo_amd.binding import GpuStore

    with GpuStore(N, [dict(name="main", alphabet="nuc", reference=data.reference.copy())]) as gpu_store:
        gpu_store.tune(TUNE_LAUNCH_COST, -1)  # (no charge per kind of launch: the block of code-plane positions is to get code planes)
        try:
            for a in range(0, N, 35_000):
                gpu_store.append_sequences(0, a, NUC_CHARS[data.sym[a:a + 35_000]])
            gpu_store.finalize()
        finally:
            gpu_store.tune(TUNE_LAUNCH_COST, 0)
        assert gpu_store.scan_runs(0) > 0  # the store derives symbols and keeps N as runs
        filters = {}
        for name, mask in data.masks.items():
            filters[name] = gpu_store.bitset_alloc()
            gpu_store.bitset_upload(filters[name], dense.pack_bits(mask))
        gpu_store.filters = filters
        yield gpu_store


@pytest.fixture(scope="module")
def exact(store, data):
    """tables[filter name] of the exact entry over the whole store, checked against the dense oracle: computed once."""
    names = list(data.masks)
    tables = store.mutations_scan_ranges([(0, 0, POSITIONS)], [store.filters[name] for name in names])[0]
    scan_symbols = list(store.scan_symbols[0])
    for name, table in zip(names, tables):
        assert np.array_equal(table, dense.mutation_counts(data.sym, data.masks[name], scan_symbols, 0, POSITIONS)), name
    return dict(zip(names, tables))


def reference_index(store, data, a=0, b=POSITIONS):
    scan_symbols = list(store.scan_symbols[0])
    return np.array([scan_symbols.index(s) if s in scan_symbols else 255 for s in data.reference[a:b]], dtype=np.uint8)


def selected_rows(store, table, reference, proportion):
    n, rows = store.mutations_select(table, reference, proportion, capacity=table.size)
    assert n == len(rows)
    return sorted(map(tuple, rows.tolist()))


def check_against_exact(store, data, pruned, want, proportion, a=0, b=POSITIONS, label=""):
    assert np.array_equal(pruned.sum(axis=1), want.sum(axis=1)), (label, proportion)
    reference = reference_index(store, data, a, b)
    assert selected_rows(store, pruned, reference, proportion) == selected_rows(store, want, reference, proportion), (label, proportion)
    # positions that derive another symbol than the reference's, or none: never pruned
    for position in [OTHER_REFERENCE, *CODE_PLANES]:
        if a <= position < b:
            assert np.array_equal(pruned[position - a], want[position - a]), (label, proportion, position)


@pytest.mark.parametrize("proportion", PROPORTIONS)
def test_selected_rows_and_row_sums_match_the_exact_scan(store, data, exact, proportion):
    names = list(data.masks)
    for name in names:  # one filter per call: k_scan_escapes_sliced<1>
        pruned = store.mutations_scan_ranges([(0, 0, POSITIONS)], [store.filters[name]], min_proportions=[proportion])[0][0]
        check_against_exact(store, data, pruned, exact[name], proportion, label=name)
        if proportion == 0:
            assert np.array_equal(pruned, exact[name]), name
    together = store.mutations_scan_ranges([(0, 0, POSITIONS)], [store.filters[name] for name in names], min_proportions=[proportion] * len(names))[0]
    for name, pruned in zip(names, together):  # five filters in one pass: a granule is skipped only where all of them allow it
        check_against_exact(store, data, pruned, exact[name], proportion, label=name + " (batch)")


def test_group_totals_on_the_bound_and_one_above(store, data, exact):
    """A group of exactly must_exceed keys is left out (<=, not <), a group of one more is counted and reported.  The all-rows
    case pins the kernel's boundary: there the lower bound of the covered rows IS the covered rows of the crafted positions
    (they have the most rows without a symbol of their granules), so the group on the bound must vanish from the table.  Under
    the 40 % filter other positions of the granule have rows without a symbol, the kernel's bound lies below the select
    kernel's and the granule stays: that case checks the select side of the boundary only (one above is reported, on it is not)."""
    scan_symbols = list(store.scan_symbols[0])
    for name, proportion, at, above, bound in (("all rows", 0.01, AT_BOUND, ABOVE_BOUND, data.bound_all),
                                               ("random 40 %", 0.05, F_AT_BOUND, F_ABOVE_BOUND, data.bound_40)):
        pruned = store.mutations_scan_ranges([(0, 0, POSITIONS)], [store.filters[name]], min_proportions=[proportion])[0][0]
        want = exact[name]
        symbol_at, symbol_above = scan_symbols.index(data.second[at]), scan_symbols.index(data.second[above])
        assert want[at, symbol_at] == bound and want[above, symbol_above] == bound + 1
        assert want[at].sum() and must_exceed(want[at].sum(), proportion) == bound  # the select kernel's own threshold at this position
        assert must_exceed(want[above].sum(), proportion) == bound
        assert pruned[above, symbol_above] == bound + 1
        rows = selected_rows(store, pruned, reference_index(store, data), proportion)
        assert (above, symbol_above, bound + 1, int(want[above].sum())) in rows
        assert not any(row[0] == at and row[1] == symbol_at for row in rows)
        if name == "all rows":  # the kernel's lower bound of the covered rows is the exact number here: the granule is skipped
            assert pruned[at, symbol_at] == 0


def test_sub_ranges_inside_granules_and_runs(store, data, exact):
    ranges = [(0, 123, 456), (0, 1, 2), (0, 97, 104), (0, 290, POSITIONS), (0, 505, 599)]
    names = ["random 40 %", "all rows"]
    for proportion in (0.01, 0.05):
        tables = store.mutations_scan_ranges(ranges, [store.filters[name] for name in names], min_proportions=[proportion] * 2)
        for (_, a, b), per_filter in zip(ranges, tables):
            for name, pruned in zip(names, per_filter):
                check_against_exact(store, data, pruned, exact[name][a:b], proportion, a, b, label=(name, a, b))


def test_eight_filters_with_their_own_proportions(store, data, exact):
    """One pass of k_scan_escapes_sliced<8>: a granule is skipped where every one of the eight filters allows it."""
    batches = [
        (["random 40 %", "all rows", "random 40 %", "all rows", "random 40 %", "all rows", "random 40 %", "all rows"],
         [0.05, 0.01, 0.5, 1.0, 0.01, 0.05, 1.0, 0.5], True),
        (["random 40 %", "all rows", "a few hundred rows", "second slice only", "random 40 %", "empty", "all rows", "random 40 %"],
         [0.05, 0.01, 0.05, 0.5, 1.0, 0.05, 0.0, 0.01], False),  # (an empty filter, a proportion of 0: nothing may be skipped)
    ]
    for names, proportions, skips in batches:
        tables = store.mutations_scan_ranges([(0, 0, POSITIONS)], [store.filters[name] for name in names], min_proportions=proportions)[0]
        for name, proportion, pruned in zip(names, proportions, tables):
            check_against_exact(store, data, pruned, exact[name], proportion, label=name)
        assert any(not np.array_equal(pruned, exact[name]) for name, pruned in zip(names, tables)) == skips


def test_knob_off_or_no_proportion_is_the_exact_table(store, data, exact):
    names = ["random 40 %", "all rows", "second slice only"]
    filters = [store.filters[name] for name in names]
    zero = store.mutations_scan_ranges([(0, 0, POSITIONS)], filters, min_proportions=[0.0] * len(names))[0]
    previous = store.tune(TUNE_PRUNE_KEYS, -1)
    try:
        off = store.mutations_scan_ranges([(0, 0, POSITIONS)], filters, min_proportions=[0.05] * len(names))[0]
    finally:
        store.tune(TUNE_PRUNE_KEYS, previous)
    on = store.mutations_scan_ranges([(0, 0, POSITIONS)], filters, min_proportions=[0.05] * len(names))[0]
    for k, name in enumerate(names):
        assert zero[k].tobytes() == exact[name].tobytes(), name
        assert off[k].tobytes() == exact[name].tobytes(), name
    assert any(not np.array_equal(on[k], exact[name]) for k, name in enumerate(names))  # (the knob is what made the difference)


def test_most_granules_are_skippable(store, data):
    cardinality = int(data.masks["random 40 %"].sum())
    skippable, total = store.scan_prunable_granules(0, cardinality, 0.05)
    assert total >= 20 and skippable > total // 2, (skippable, total)
    assert store.scan_prunable_granules(0, cardinality, 0.0) == (0, total)
    assert store.scan_prunable_granules(0, 0, 0.05) == (0, total)


# ---- engine level --------------------------------------------------------------------------------------------------------------
PART_ROWS = 66_000  # a partition's stores are re-encoded (derived symbols, gap events, bounds) from 65 536 rows on
ENGINE_STORES = {  # name: (amino acids?, positions, letters, missing, ambiguity code, position whose most numerous symbol is not the
                   # reference's, positions with a substitution in 8 % of the rows, position of the group split over two partitions)
    "main": (False, 300, "ACGT", "N", "R", 60, (10, 130), 200),
    "S": (True, 120, "ACDEFGHIKLMNPQRSTVWY", "X", "B", 30, (5, 80), 50),
}
SPLIT_GROUP = (600, 2300)  # rows of the split group inside the filter, per partition: together reported at 0.05, the second part alone not
TUNE_SCAN_TIMING = 7


def engine_of(n_partitions):
    """Settled stores as in the store fixture — the reference symbol in nearly every row, a second one in 0.2 %, runs of the
    missing symbol, ambiguity codes — in `n_partitions` parts of PART_ROWS rows; returns the engine, the references, the buckets
    of the rows (the queries filter on bucket <= 3) and the names of the split groups' mutations."""
    from silo_amd.engine import Engine

    rng = np.random.default_rng(59)
    rows = PART_ROWS * n_partitions
    bucket = rng.integers(0, 10, size=rows)
    references, sequences, split_mutations = {}, {}, {}
    for name, (_, positions, letters, missing, code, other_reference, substituted, split) in ENGINE_STORES.items():
        alphabet = np.frombuffer(letters.encode(), dtype=np.uint8)
        reference_index = rng.integers(0, len(alphabet), size=positions)
        reference = alphabet[reference_index]
        second = alphabet[(reference_index + 1) % len(alphabet)]
        third = alphabet[(reference_index + 2) % len(alphabet)]
        draw = rng.random((rows, positions), dtype=np.float32)
        chars = np.where(draw < 0.002, second, reference)
        chars = np.where((draw >= 0.002) & (draw < 0.0022), third, chars)
        chars = np.where((draw >= 0.0022) & (draw < 0.0027), np.uint8(ord(code)), chars).astype(np.uint8)
        for row in rng.choice(rows, size=600 * n_partitions, replace=False):
            start = int(rng.integers(0, positions))
            chars[row, start:start + int(rng.geometric(1 / 40))] = ord(missing)
        for p in substituted:  # reported at 0.05
            chars[rng.random(rows) < 0.08, p] = third[p]
        chars[rng.random(rows) < 0.6, other_reference] = second[other_reference]  # reported at 0.5; derives another symbol than the reference's
        chars[:, split] = reference[split]
        for k in range(n_partitions):  # few keys of the group in the first partition, many in the second
            inside = k * PART_ROWS + np.flatnonzero(bucket[k * PART_ROWS:(k + 1) * PART_ROWS] <= 3)
            chars[rng.permutation(inside)[:SPLIT_GROUP[k]], split] = second[split]
        references[name] = bytes(reference).decode()
        sequences[name] = [bytes(row).decode() for row in chars]
        split_mutations[name] = f"{chr(reference[split])}{split + 1}{chr(second[split])}"
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": references["main"]}], "genes": [{"name": "S", "sequence": references["S"]}]})
    engine.set_schema("key", "date")
    for k in range(n_partitions):
        lo, hi = k * PART_ROWS, (k + 1) * PART_ROWS
        part = engine.add_partition(PART_ROWS)
        for name, (is_aa, *_rest) in ENGINE_STORES.items():
            engine.append_sequences(part, name, is_aa, 0, sequences[name][lo:hi])
        engine.append_metadata(part, "key", "string", [str(i) for i in range(lo, hi)])
        engine.append_metadata(part, "date", "date", ["2021-03-04"] * PART_ROWS)
        engine.append_metadata(part, "bucket", "int", [str(b) for b in bucket[lo:hi]])
    engine.finalize()
    return engine, bucket, split_mutations


@pytest.mark.parametrize("n_partitions", [1, 2])
def test_engine_bodies_do_not_depend_on_the_knob(built, n_partitions):
    """One partition: the scans of Mutations and AminoAcidMutations prune (the launch says so, the stores have granules to skip)
    and the bodies are those of the exact scans.  Two partitions: no scan prunes — the first partition's part of the split
    group, small against that partition's filter, is needed for the row the two parts give together."""
    from silo_amd import binding

    lib = binding.load_library()
    lib.silo_gpu_tune(TUNE_LAUNCH_COST, -1)
    try:
        engine, bucket, split_mutations = engine_of(n_partitions)
    finally:
        lib.silo_gpu_tune(TUNE_LAUNCH_COST, 0)
    # every partition's stores derive symbols and have granules of keys that the filter's rows of that partition would skip
    for k in range(n_partitions):
        view = engine.partition_store(k)
        cardinality = int((bucket[k * PART_ROWS:(k + 1) * PART_ROWS] <= 3).sum())
        for name, (is_aa, *_rest) in ENGINE_STORES.items():
            skippable, total = ctypes_u64(), ctypes_u64()
            binding._check(lib.silo_gpu_store_scan_prunable_granules(view.handle, engine.seqstore_id(k, name, is_aa), cardinality, 0.05, skippable, total))
            assert total.value >= 4 and skippable.value > 0, (k, name, skippable.value, total.value)
    queries = [
        (action, proportion, json.dumps({"action": {"type": action, "minProportion": proportion},
                                         "filterExpression": {"type": "IntBetween", "column": "bucket", "from": 0, "to": 3}}))
        for action in ("Mutations", "AminoAcidMutations") for proportion in (0.05, 0.5)
    ]
    bodies, pruning = {}, {}
    for value in (0, -1):
        previous = lib.silo_gpu_tune(TUNE_PRUNE_KEYS, value)
        lib.silo_gpu_tune(TUNE_SCAN_TIMING, 1)
        try:
            bodies[value], pruning[value] = [], []
            for _, _, query in queries:
                bodies[value].append(engine.execute_text(query))
                pruning[value].append(any(", pruning" in entry["kernel"] for entry in binding.scan_timings()))  # (the query's last scan)
        finally:
            lib.silo_gpu_tune(TUNE_SCAN_TIMING, 0)
            lib.silo_gpu_tune(TUNE_PRUNE_KEYS, previous)
    assert all(status == 200 for status, _ in bodies[0]), bodies[0]
    assert pruning[-1] == [False] * len(queries)
    assert pruning[0] == [n_partitions == 1] * len(queries)  # the action's proportion reaches the scan; never with two scans into one table
    assert bodies[0] == bodies[-1]
    for (action, proportion, _), (_, body) in zip(queries, bodies[0]):
        rows = {row["mutation"]: row["count"] for row in json.loads(body)["queryResult"]}
        assert rows, (action, proportion)
        if proportion == 0.05:  # the split group: reported with both parts where there are two, too small by itself
            mutation = split_mutations["main" if action == "Mutations" else "S"]
            assert rows.get(mutation) == (sum(SPLIT_GROUP) if n_partitions == 2 else None), (action, mutation)


def ctypes_u64():
    import ctypes

    return ctypes.c_uint64(0)
