"""The Mutations scan that may leave out one-hot plane ROWS below a filter's minProportion
(silo_gpu_mutations_scan_ranges_min_proportion, k_scan_sliced<2, 2, ..., KIND_ROWS> walking a list of live rows): row sums, the
rows silo_gpu_mutations_select reports and the cells of the one-hot rows, against the exact entry and the dense oracle."""
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

N, POSITIONS = 140_000, 200  # two slices of 2^17 rows, the second partial; not a multiple of 2048 rows; above 65 536 rows
ROW_BYTES = (N + 2047) // 2048 * 256  # rows are padded to 32 words
KEY_COST_BYTES = 10                   # a symbol gets a row once its keys would cost more than the row: from N / 80 = 1 750 rows on
SECOND_SHARE = (0.015, 0.03, 0.08)    # of the rows, by position % 3: a one-hot row each
THIRD_SHARE = 0.02                    # at every fourth position a third symbol: two rows at that position
AT_BOUND, ABOVE_BOUND = 100, 150      # under the all-rows filter at 0.05: a row of exactly must_exceed rows, and of one more
OTHER_REFERENCE = 60                  # the most numerous symbol is not the reference symbol: the reference symbol has the row
CODE_PLANES = range(180, 192)         # five symbols a fifth of the rows each: three identity code planes, nothing derived
SHARED = 120                          # the reference symbol in 40 % of the rows, two others in 35 % and 25 %: two rows, never left out
AMBIGUOUS_AT_CRAFTED = 5000


def must_exceed(covered, proportion):
    return int(math.ceil(float(covered) * proportion) - 1)


def prunable(cardinality, without, heaviest, proportion):
    """granulePrunable of store_internal.h."""
    if not proportion > 0 or proportion > 1 or cardinality <= without:
        return False
    return heaviest <= must_exceed(cardinality - without, proportion)


class Built:
    pass


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(61)
    valid = np.array([0, 1, 2, 3, 4])
    orders = np.array([rng.permutation(valid) for _ in range(POSITIONS)], dtype=np.uint8)
    dominant, second, third = orders[:, 0].copy(), orders[:, 1].copy(), orders[:, 2].copy()
    second_share = np.array([SECOND_SHARE[p % 3] for p in range(POSITIONS)], dtype=np.float32)
    third_share = np.array([THIRD_SHARE if p % 4 == 1 else 0.0002 for p in range(POSITIONS)], dtype=np.float32)
    draw = rng.random((N, POSITIONS), dtype=np.float32)
    sym = np.where(draw < second_share, second, dominant).astype(np.uint8)
    sym = np.where((draw >= second_share) & (draw < second_share + third_share), third, sym)
    lone = (draw >= 0.9) & (draw < 0.901)  # other symbols in 0.1 %: escape keys, ambiguity codes
    sym[lone] = rng.integers(0, 16, size=int(lone.sum()))
    del draw
    rows = rng.choice(N, size=1500, replace=False)
    for k, row in enumerate(rows):  # runs of N, some from position 0, ambiguity codes beside them
        for _ in range(1 + k % 3):
            start = 0 if k % 7 == 0 else int(rng.integers(0, POSITIONS))
            end = min(POSITIONS, start + int(rng.geometric(1 / 60)))
            sym[row, start:end] = N_SYMBOL
            if k % 5 == 0 and end < POSITIONS:
                sym[row, end] = rng.choice(AMBIGUITY_CODES)
    sym[rng.choice(N, size=N // 1000, replace=False)] = N_SYMBOL  # rows missing throughout
    # the boundary: covered = N - 5 000 at both positions, one row each
    bound_all = must_exceed(N - AMBIGUOUS_AT_CRAFTED, 0.05)
    for position, total in ((AT_BOUND, bound_all), (ABOVE_BOUND, bound_all + 1)):
        chosen = rng.permutation(N)
        sym[:, position] = dominant[position]
        sym[chosen[total:total + AMBIGUOUS_AT_CRAFTED], position] = AMBIGUITY_CODES[position % len(AMBIGUITY_CODES)]
        sym[chosen[:total], position] = second[position]
    for position in CODE_PLANES:  # (a fifth symbol as keys would cost more than the third plane: rows for three of four lose too)
        sym[:, position] = valid[rng.integers(0, 5, size=N)]
    share = rng.random(N)
    sym[:, SHARED] = np.where(share < 0.4, dominant[SHARED], np.where(share < 0.75, second[SHARED], third[SHARED]))
    reference = dominant.copy()
    reference[OTHER_REFERENCE] = second[OTHER_REFERENCE]
    one_slice = (np.arange(N) >> 17) == 1
    # five rows in each of 60 of the filter's 64-byte sectors (512 rows): few enough sectors for the gather route
    few_hundred = np.zeros(N, bool)
    for sector in rng.choice(N // 512, size=60, replace=False):
        few_hundred[sector * 512 + rng.choice(512, size=5, replace=False)] = True
    masks = {
        "random 40 %": rng.random(N) < 0.4,
        "a few hundred rows": few_hundred,
        "empty": np.zeros(N, bool),
        "second slice only": one_slice & (rng.random(N) < 0.8),
        "all rows": np.ones(N, bool),
    }
    built = Built()
    built.sym, built.reference, built.masks, built.bound_all = sym, reference, masks, bound_all
    built.dominant, built.second = dominant, second
    return built


@pytest.fixture(scope="module")
def store(built, data):
    from silo_amd.binding import GpuStore

    with GpuStore(N, [dict(name="main", alphabet="nuc", reference=data.reference.copy())]) as gpu_store:
        gpu_store.tune(TUNE_LAUNCH_COST, -1)  # (no charge per kind of launch: the block of CODE_PLANES is to get its code planes)
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


@pytest.fixture(scope="module")
def model(store, data, exact):
    """What the test knows of the store's one-hot rows from the data alone: is_row[p, s] (a symbol other than the most numerous one
    whose keys would cost more than a row, outside the block of code planes), may_go[p] (the derived symbol is the reference
    symbol), without[p] (rows without a valid symbol), totals[p, s]."""
    scan_symbols = list(store.scan_symbols[0])
    built = Built()
    built.totals = exact["all rows"].astype(np.int64)
    built.without = N - built.totals.sum(axis=1)
    built.is_row = built.totals * KEY_COST_BYTES > ROW_BYTES
    built.may_go = np.zeros(POSITIONS, bool)
    for p in range(POSITIONS):
        built.is_row[p, scan_symbols.index(data.dominant[p])] = False
        # (the derived symbol is the reference's and holds the majority of the position's valid rows)
        built.may_go[p] = data.reference[p] == data.dominant[p] and 2 * built.totals[p, scan_symbols.index(data.dominant[p])] > built.totals[p].sum()
    built.is_row[list(CODE_PLANES)] = False
    built.may_go[list(CODE_PLANES)] = False
    return built


def skipped_rows(model, cardinalities, proportions):
    """skipped[p, s]: the one-hot rows that EVERY (cardinality, proportion) allows to leave out."""
    skipped = np.zeros_like(model.is_row)
    for p, s in zip(*np.nonzero(model.is_row)):
        skipped[p, s] = model.may_go[p] and all(
            prunable(c, int(model.without[p]), int(model.totals[p, s]), q) for c, q in zip(cardinalities, proportions))
    return skipped


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
    # never pruned: a position whose derived symbol is not the reference's, one that several symbols share, the block of code planes
    for position in [OTHER_REFERENCE, SHARED, *CODE_PLANES]:
        if a <= position < b:
            assert np.array_equal(pruned[position - a], want[position - a]), (label, proportion, position)


def check_row_cells(pruned, want, is_row, skipped, label=""):
    """The cells of the one-hot rows: zero where the row was left out, exact where it was walked."""
    assert np.array_equal(pruned[is_row & ~skipped], want[is_row & ~skipped]), label
    assert not pruned[skipped].any(), label


def scan(store, names, proportions, ranges=((0, 0, POSITIONS),)):
    return store.mutations_scan_ranges(list(ranges), [store.filters[name] for name in names], min_proportions=list(proportions))


def test_the_store_has_the_rows_the_data_asks_for(store, data, model):
    """(The model of the layout that the other tests lean on.)"""
    assert store.scan_prunable_rows(0, N, 0.05)[1] == int(model.is_row.sum())  # (none of them in the block of code planes)
    assert model.is_row[OTHER_REFERENCE].sum() == 1 and not model.may_go[OTHER_REFERENCE]
    assert model.is_row[SHARED].sum() == 2 and not model.may_go[SHARED] and data.reference[SHARED] == data.dominant[SHARED]
    assert prunable(N, int(model.without[SHARED]), int(model.totals[SHARED].max()), 0.5)  # (the plain rule would let its rows go)
    assert (model.is_row.sum(axis=1) == 2).sum() >= 40 and model.is_row[0].sum() == 1 and model.is_row[1].sum() == 2


@pytest.mark.parametrize("proportion", PROPORTIONS)
def test_selected_rows_and_row_sums_match_the_exact_scan(store, data, exact, model, proportion):
    names = list(data.masks)
    for name in names:  # one filter per call: k_scan_sliced<2, 2, 8, 1, 2>
        pruned = scan(store, [name], [proportion])[0][0]
        check_against_exact(store, data, pruned, exact[name], proportion, label=name)
        if proportion == 0:
            assert pruned.tobytes() == exact[name].tobytes(), name
        if name in ("all rows", "random 40 %"):  # (dense filters: the row kernel counts them)
            skipped = skipped_rows(model, [int(data.masks[name].sum())], [proportion])
            check_row_cells(pruned, exact[name], model.is_row, skipped, (name, proportion))
        else:  # the gather route counts every row; an empty filter vetoes
            assert np.array_equal(pruned[model.is_row], exact[name][model.is_row]), (name, proportion)
    together = scan(store, names, [proportion] * len(names))[0]
    for name, pruned in zip(names, together):  # five filters in one pass, the empty one among them: no row is left out
        check_against_exact(store, data, pruned, exact[name], proportion, label=name + " (batch)")
        assert np.array_equal(pruned[model.is_row], exact[name][model.is_row]), (name, proportion)


def test_row_totals_on_the_bound_and_one_above(store, data, exact, model):
    """A row of exactly must_exceed rows is left out (<=, not <), a row of one more is counted and reported; `without` of a row is
    that of its own position, so the kernel's covered rows are the select kernel's under the all-rows filter."""
    scan_symbols = list(store.scan_symbols[0])
    want = exact["all rows"]
    pruned = scan(store, ["all rows"], [0.05])[0][0]
    symbol_at, symbol_above = scan_symbols.index(data.second[AT_BOUND]), scan_symbols.index(data.second[ABOVE_BOUND])
    assert model.is_row[AT_BOUND, symbol_at] and model.is_row[ABOVE_BOUND, symbol_above]
    assert want[AT_BOUND, symbol_at] == data.bound_all and want[ABOVE_BOUND, symbol_above] == data.bound_all + 1
    assert model.without[AT_BOUND] == AMBIGUOUS_AT_CRAFTED and model.without[ABOVE_BOUND] == AMBIGUOUS_AT_CRAFTED
    assert must_exceed(want[AT_BOUND].sum(), 0.05) == data.bound_all and must_exceed(want[ABOVE_BOUND].sum(), 0.05) == data.bound_all
    assert pruned[AT_BOUND, symbol_at] == 0
    assert pruned[ABOVE_BOUND, symbol_above] == data.bound_all + 1
    rows = selected_rows(store, pruned, reference_index(store, data), 0.05)
    assert (ABOVE_BOUND, symbol_above, data.bound_all + 1, int(want[ABOVE_BOUND].sum())) in rows
    assert not any(row[0] == AT_BOUND and row[1] == symbol_at for row in rows)


def test_list_shapes(store, data, exact, model):
    """An odd number of live rows, every row of the range left out, none left out; ranges that begin at the second row of a pair
    and a range of one position with two rows."""
    want = exact["all rows"]
    skipped = skipped_rows(model, [N], [0.05])
    assert skipped.any() and (model.is_row & ~skipped).any()
    live_before = np.concatenate([[0], np.cumsum((model.is_row & ~skipped).sum(axis=1))])
    rows_before = np.concatenate([[0], np.cumsum(model.is_row.sum(axis=1))])
    odd_end = next(b for b in range(20, 170) if live_before[b] % 2 == 1 and rows_before[b] % 2 == 0 and skipped[:b].any())
    even_end = next(b for b in range(20, 170) if live_before[b] % 2 == 0 and rows_before[b] % 2 == 1 and skipped[:b].any())
    two_rows = next(p for p in range(2, 170) if model.is_row[p].sum() == 2 and skipped[p].sum() == 1)
    assert model.is_row[0].sum() == 1 and model.is_row[1].sum() == 2  # (0, 1, 2) begins at the second row of the store's first pair
    ranges = [(0, 0, odd_end), (0, 0, even_end), (0, 1, 2), (0, two_rows, two_rows + 1), (0, 1, odd_end), (0, 3, 59)]
    for (_, a, b), per_filter in zip(ranges, scan(store, ["all rows"], [0.05], ranges)):
        check_against_exact(store, data, per_filter[0], want[a:b], 0.05, a, b, label=(a, b))
        check_row_cells(per_filter[0], want[a:b], model.is_row[a:b], skipped[a:b], (a, b))
    # every row of the range left out (its blocks leave before their first plane load), and none
    a, b = 3, 59  # (no position that keeps its rows whatever the proportion)
    for proportion, all_or_none in ((1.0, True), (0.5, True), (0.01, False)):
        pruned = scan(store, ["all rows"], [proportion], [(0, a, b)])[0][0]
        check_against_exact(store, data, pruned, want[a:b], proportion, a, b, label=proportion)
        gone = skipped_rows(model, [N], [proportion])[a:b][model.is_row[a:b]]
        assert gone.all() if all_or_none else not gone.any()
        if all_or_none:
            assert not pruned[model.is_row[a:b]].any(), proportion
        else:
            assert np.array_equal(pruned[model.is_row[a:b]], want[a:b][model.is_row[a:b]]), proportion


def test_eight_filters_with_their_own_proportions(store, data, exact, model):
    """One pass of k_scan_sliced<2, 2, 4, 8, 2>: a row is left out only where every one of the eight filters allows it."""
    names = ["random 40 %", "all rows"] * 4
    proportions = [0.05, 0.05, 0.5, 1.0, 0.5, 0.08, 1.0, 0.5]
    cardinalities = [int(data.masks[name].sum()) for name in names]
    skipped = skipped_rows(model, cardinalities, proportions)
    alone = skipped_rows(model, [N], [0.08])
    assert skipped.any() and (alone & ~skipped).any()  # (rows that one filter would let go and another keeps)
    tables = scan(store, names, proportions)[0]
    for name, proportion, pruned in zip(names, proportions, tables):
        check_against_exact(store, data, pruned, exact[name], proportion, label=name)
        check_row_cells(pruned, exact[name], model.is_row, skipped, (name, proportion))
    # an empty filter, a proportion of 0: nothing may be skipped, neither rows nor keys
    for names, proportions in (
        (["random 40 %", "all rows", "a few hundred rows", "second slice only", "random 40 %", "empty", "all rows", "random 40 %"],
         [0.05, 0.05, 0.05, 0.5, 1.0, 0.05, 0.5, 0.05]),
        (["random 40 %", "all rows", "random 40 %", "all rows", "random 40 %", "all rows", "all rows", "random 40 %"],
         [0.05, 0.05, 0.5, 0.5, 1.0, 1.0, 0.0, 0.05]),
    ):
        for name, pruned in zip(names, scan(store, names, proportions)[0]):
            assert pruned.tobytes() == exact[name].tobytes(), (name, proportions)
    # a filter that takes the gather route has no say: the dense filters' rows go, its own table stays exact
    names, proportions = ["all rows", "a few hundred rows", "random 40 %"], [0.5, 0.01, 0.5]
    skipped = skipped_rows(model, [N, int(data.masks["random 40 %"].sum())], [0.5, 0.5])
    assert skipped.any()
    tables = scan(store, names, proportions)[0]
    for name, proportion, pruned in zip(names, proportions, tables):
        check_against_exact(store, data, pruned, exact[name], proportion, label=name)
    check_row_cells(tables[0], exact[names[0]], model.is_row, skipped, names[0])
    check_row_cells(tables[2], exact[names[2]], model.is_row, skipped, names[2])
    assert np.array_equal(tables[1][model.is_row], exact[names[1]][model.is_row])


def test_knobs(store, data, exact, model):
    names = ["random 40 %", "all rows"]
    tables = {}
    for value in (-1, 1, 0):
        previous = store.tune(TUNE_PRUNE_KEYS, value)
        try:
            tables[value] = scan(store, names, [0.05, 0.05])[0]
        finally:
            store.tune(TUNE_PRUNE_KEYS, previous)
    for k, name in enumerate(names):
        assert tables[-1][k].tobytes() == exact[name].tobytes(), name
        # keys only: every one-hot row is walked, as before rows could be left out
        assert np.array_equal(tables[1][k][model.is_row], exact[name][model.is_row]), name
        check_against_exact(store, data, tables[1][k], exact[name], 0.05, label=name)
    assert any(not np.array_equal(tables[0][k][model.is_row], tables[1][k][model.is_row]) for k in range(len(names)))


def test_host_count_of_skippable_rows(store, data, model):
    total = int(model.is_row.sum())
    assert store.scan_prunable_rows(0, N, 0.0) == (0, total)
    assert store.scan_prunable_rows(0, 0, 0.05) == (0, total)
    for name, proportion in (("all rows", 0.05), ("random 40 %", 0.05), ("all rows", 0.01), ("all rows", 1.0)):
        cardinality = int(data.masks[name].sum())
        assert store.scan_prunable_rows(0, cardinality, proportion) == (int(skipped_rows(model, [cardinality], [proportion]).sum()), total)
    assert store.scan_prunable_rows(0, N, 0.05)[0] > 0
