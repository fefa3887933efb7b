"""The Mutations scan over AMINO-ACID stores with derived symbols: 22 scan symbols, the stop codon at symbol id 23 and scan index
21 with the ambiguity codes B and Z in between, the missing symbol X.  Three stores of different lengths in ONE call — as
AminoAcidMutations scans its genes — through the exact entry, the pruning entry and the entry that selects its rows in the finish
kernel (k_finish_scan<true, 22>), every table against oracle.dense.mutation_counts on the generated symbols.  The long store has
a stretch with so few keys that its granules span more than the escape pass's counter window: keys on the overflow list."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import scan_alignments as sa  # noqa: E402
from tests.scan_alignments import GAP  # noqa: E402

N = 131_200  # two slices of 2^17 rows, the second of 128 rows; rows of 2 080 words: the finish kernel may select
GENES = [("short", 75), ("block", 1_024), ("long", 1_300)]  # a partial finish block; exactly one; two
SHORT, BLOCK, LONG = 0, 1, 2
TABLE_OFFSET = [0, 75, 1_099]
TOTAL_POSITIONS = 2_399
WHOLE = [(SHORT, 0, 75), (BLOCK, 0, 1_024), (LONG, 0, 1_300)]
QUIET = (200, 1_100)  # codons of `long` with exactly two keyed rows per position and slice
CODE_PLANES = range(800, 812)  # of `block`: six symbols a sixth of the rows each — three code planes, nothing derived
PROPORTIONS = (0.0, 0.01, 0.05, 0.5, 1.0)
# crafted groups of exactly must_exceed rows (AT) and of one more (ABOVE): (store, position, filter, proportion, one more?)
CRAFTED = [
    (BLOCK, 300, "all rows", 0.01, False), (BLOCK, 500, "all rows", 0.01, True),
    (BLOCK, 600, "random 40 %", 0.05, False), (BLOCK, 700, "random 40 %", 0.05, True),
    # inside the quiet stretch: whichever way the granules of slice 0 fall, the keys of 640 or of 1 060 lie more than 272 codons
    # behind their granule's first
    (LONG, 640, "all rows", 0.01, True), (LONG, 650, "all rows", 0.01, False), (LONG, 1_060, "all rows", 0.01, True),
]
ROLES = {  # positions where the stop codon and the gap symbol play a given part
    "short": dict(stop_row=30, stop_derived=35, stop_other_reference=38, stop_rare=40, stop_reference=42, gap_row=37, gap_derived=33, small_rows=[36]),
    "block": dict(stop_row=200, stop_derived=210, stop_other_reference=220, stop_rare=230, stop_reference=240, gap_row=260, gap_derived=270,
                  small_rows=list(range(310, 350, 4))),
    "long": dict(stop_row=1_120, stop_derived=100, stop_other_reference=1_150, stop_rare=120, stop_reference=130, gap_row=140, gap_derived=160,
                 small_rows=[170, 1_110, 1_130]),
}
GAP_ROWS = [77, 131_072 + 5]                # the gap symbol throughout, one row per slice
MISSING_ROWS = [1_234, 90_001, 131_072 + 100]  # the missing symbol throughout
QUIET_POOL = ([11, 5_003, 40_007, 77_777, 100_003, 131_000], [131_072 + 17, 131_072 + 64, 131_072 + 127])  # rows that carry the stretch's keys, per slice
KEYS = sa.KEY_COST_BYTES
FILTERS = ["random 40 %", "a few hundred rows", "empty", "all rows", "second slice only", "first slice only", "rows >= 60 %", "random 90 %"]


class Built:
    pass


def make_gene(rng, symbols, name, positions, free_rows, masks):
    """The symbols of one gene uint8 [N][positions], its reference, and the crafted groups' sizes."""
    stop, missing = symbols.symbol("*"), symbols.missing
    spare = [symbols.symbol(c) for c in "ACD"]
    roles = ROLES[name]
    dominant, second, third = sa.symbol_orders(rng, symbols, positions)
    second_share = np.full(positions, 0.002, dtype=np.float32)
    third_share = np.full(positions, 0.0002, dtype=np.float32)

    def assign(position, first, other, share):
        dominant[position], second[position] = first, other
        third[position] = next(s for s in spare if s not in (first, other))
        second_share[position] = share

    letter = spare[0]
    assign(roles["stop_row"], letter, stop, 0.05)               # second most frequent: a one-hot row
    assign(roles["stop_derived"], stop, letter, 0.002)          # most numerous and the reference symbol
    assign(roles["stop_other_reference"], stop, letter, 0.05)   # most numerous, the reference symbol has the row
    assign(roles["stop_rare"], letter, stop, 0.002)             # escape keys
    assign(roles["stop_reference"], letter, stop, 0.05)         # the reference symbol, with a row
    for position in roles["small_rows"]:                        # a one-hot row of 1.5 % of the rows: left out at 0.05 under the 40 % filter
        second_share[position] = 0.015
    if name == "long":
        second_share[QUIET[0]:QUIET[1]] = 0
        third_share[QUIET[0]:QUIET[1]] = 0
    sym = sa.settled_positions(rng, symbols, N, dominant, second, third, second_share, third_share)
    reference = dominant.copy()
    reference[roles["stop_other_reference"]] = letter
    reference[roles["stop_reference"]] = stop
    reference[0] = GAP  # (the ragged ends make the gap symbol the most numerous one there)
    # ragged ends in 70 % of the rows, runs of X (in `long` some across codon 1 023 / 1 024), codes beside them
    ragged = free_rows[rng.random(len(free_rows)) < 0.7]
    end_mean = 5 if name == "short" else 25  # (of 75 codons the ends are to leave most to their letters)
    sa.add_ragged_ends(rng, sym, ragged, end_mean, end_mean, min(150, positions))
    with_runs = rng.choice(free_rows, size=1_500, replace=False)
    sa.add_missing_runs(rng, symbols, sym, with_runs, 150, crossing=[((900, 1_020), (1_030, 1_200), 60)] if name == "long" else ())
    sym[rng.random(N) < 0.3, roles["gap_row"]] = GAP      # interior deletions: a row of '-' that no end run covers
    sym[rng.random(N) < 0.6, roles["gap_derived"]] = GAP  # '-' the most numerous symbol away from the ends
    if name == "block":
        six = np.r_[symbols.letters[:4], stop, GAP].astype(np.uint8)
        for position in CODE_PLANES:
            sym[:, position] = rng.permutation(six)[rng.integers(0, 6, size=N)]
    sym[GAP_ROWS] = GAP
    sym[MISSING_ROWS] = missing
    if name == "long":  # the stretch's keys: the rows of '-' throughout, and per position and slice one row of the pool with another symbol
        for position in range(*QUIET):
            for pool in QUIET_POOL:
                others = symbols.letters[symbols.letters != dominant[position]]
                sym[pool[int(rng.integers(0, len(pool)))], position] = others[int(rng.integers(0, len(others)))]
    bounds = {}
    for store, position, filter_name, proportion, one_more in CRAFTED:
        if GENES[store][0] != name:
            continue
        mask = masks[filter_name]
        covered = int(symbols.is_valid[sym[mask, position]].sum())
        bound = sa.must_exceed(covered, proportion)
        eligible = rng.permutation(free_rows[mask[free_rows]])
        sa.craft_group(symbols, sym, position, dominant[position], second[position], eligible, bound + (1 if one_more else 0))
        bounds[position] = (bound, int(second[position]))
    return sym, reference, dominant, bounds


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(101)
    symbols = sa.Symbols("aa")
    rows = np.arange(N)
    u = rng.random(N)
    share = np.digitize(u, [0.003, 0.4, 0.7, 0.9])  # 0: 0.3 % of the rows, 1: up to 40 %, 2: up to 70 %, 3: up to 90 %, 4: the rest
    region = np.where(rows >= 131_072, 2, np.where(rows >= int(0.6 * N), 1, 0))
    classes = sa.RowClasses(share * 3 + region)
    classes.add("random 40 %", lambda label: label // 3 <= 1)
    classes.add("a few hundred rows", lambda label: label // 3 == 0)
    classes.add("empty", lambda label: False)
    classes.add("all rows", lambda label: True)
    classes.add("second slice only", lambda label: label % 3 == 2 and label // 3 <= 3)
    classes.add("first slice only", lambda label: label % 3 != 2 and label // 3 in (1, 2))
    classes.add("rows >= 60 %", lambda label: label % 3 >= 1 and label // 3 <= 2)
    classes.add("random 90 %", lambda label: label // 3 <= 3)
    assert classes.names() == FILTERS
    masks = {name: classes.mask(name) for name in FILTERS}
    reserved = np.r_[GAP_ROWS, MISSING_ROWS, QUIET_POOL[0], QUIET_POOL[1]]
    free_rows = np.setdiff1d(rows, reserved)
    made = Built()
    made.symbols, made.classes, made.masks = symbols, classes, masks
    made.sym, made.reference, made.dominant, made.bounds = [], [], [], []
    for name, positions in GENES:
        sym, reference, dominant, bounds = make_gene(rng, symbols, name, positions, free_rows, masks)
        made.sym.append(sym)
        made.reference.append(reference)
        made.dominant.append(dominant)
        made.bounds.append(bounds)
    scan_symbols = symbols.valid.tolist()
    made.want = [classes.oracle_tables(sym, scan_symbols) for sym in made.sym]  # [store][filter name]: computed once, never changed
    made.reference_index = [sa.reference_index(scan_symbols, reference) for reference in made.reference]
    # positions whose most numerous symbol is not the reference symbol, or that derive nothing: their cells are never left out
    made.never_pruned = []
    for store in range(3):
        total = made.want[store]["all rows"]
        never = set(np.flatnonzero(total.argmax(axis=1) != made.reference_index[store]).tolist())
        made.never_pruned.append(sorted(never | (set(CODE_PLANES) if store == BLOCK else set())))
    return made


@pytest.fixture(scope="module")
def store(built, data):
    from silo_amd.binding import GpuStore

    genes = [dict(name=name, alphabet="aa", reference=data.reference[k].copy()) for k, (name, _) in enumerate(GENES)]
    with GpuStore(N, genes) as gpu_store:
        assert gpu_store.row_words >= 1_024
        assert list(gpu_store.scan_symbols[0]) == data.symbols.valid.tolist()
        gpu_store.tune(sa.TUNE_LAUNCH_COST, -1)  # (no charge per kind of launch: the block of CODE_PLANES is to get its code planes)
        try:
            for k in range(3):
                for a in range(0, N, 33_333):  # (no chunk begins at a multiple of 64 rows)
                    gpu_store.append_sequences(k, a, data.symbols.chars[data.sym[k][a:a + 33_333]])
            gpu_store.finalize()
        finally:
            gpu_store.tune(sa.TUNE_LAUNCH_COST, 0)
        gpu_store.filters = dict(zip(FILTERS, sa.upload(gpu_store, [data.masks[name] for name in FILTERS])))
        yield gpu_store


def table_of(per_store):
    """The three stores' tables as the one table of TOTAL_POSITIONS positions."""
    return np.concatenate(per_store, axis=0)


# ---- the data and the store have what the tests below rely on ----------------------------------------------------------------------
def test_the_alignment_has_every_part_to_play(data):
    symbols = data.symbols
    stop, stop_index = symbols.symbol("*"), symbols.scan_index(symbols.symbol("*"))
    assert (stop, stop_index, symbols.missing, symbols.n_scan) == (23, 21, 24, 22)
    assert symbols.ambiguity.tolist() == [21, 22]  # B and Z lie between the last letter and the stop codon
    row = sa.row_bytes(N)
    for store, (name, positions) in enumerate(GENES):
        sym, roles = data.sym[store], ROLES[name]
        total = data.want[store]["all rows"].astype(np.int64)
        reference = data.reference_index[store].astype(np.int64)
        most = total.argmax(axis=1)
        ranked = np.argsort(-total, axis=1, kind="stable")
        assert (most == reference).mean() > 0.8  # settled positions that derive their reference symbol
        lead, trail_start = sa.end_runs_of(sym)
        assert 0.6 < (lead > 0).mean() < 0.8 and 0.6 < (trail_start < positions).mean() < 0.8
        assert (sym[GAP_ROWS] == GAP).all() and (sym[MISSING_ROWS] == symbols.missing).all()
        is_missing = sym == symbols.missing
        is_code = (sym == symbols.ambiguity[0]) | (sym == symbols.ambiguity[1])
        assert is_missing[:, 0].sum() > len(MISSING_ROWS) + 50  # runs from codon 0
        assert (is_code[:, 1:] & is_missing[:, :-1]).sum() > 50 and (is_code[:, :-1] & is_missing[:, 1:]).sum() > 50  # codes beside runs
        assert (is_code[:, 1:-1] & ~is_missing[:, :-2] & ~is_missing[:, 2:]).sum() > 50  # and alone

        def has_row(p, symbol):  # its keys would cost more than a row
            return KEYS * total[p, symbol] > row

        def outside_end_runs(p):  # rows of '-' at p that no end run holds
            return total[p, 0] - int((lead > p).sum() + (trail_start <= p).sum())

        p = roles["stop_row"]
        assert ranked[p, 1] == stop_index and has_row(p, stop_index)
        p = roles["stop_derived"]
        assert most[p] == stop_index == reference[p]
        p = roles["stop_other_reference"]
        assert most[p] == stop_index != reference[p] and has_row(p, reference[p])
        p = roles["stop_rare"]
        assert 0 < total[p, stop_index] and not has_row(p, stop_index) and most[p] != stop_index
        p = roles["stop_reference"]
        assert reference[p] == stop_index != most[p]
        p = roles["gap_row"]  # a row that no end run covers: its bits outside the end runs would cost more as keys than the row
        assert most[p] != 0 and has_row(p, 0) and KEYS * outside_end_runs(p) >= row
        p = roles["gap_derived"]
        assert most[p] == 0 != reference[p]
        assert most[0] == 0 == reference[0]  # most numerous at the ragged end, and the reference symbol there
        assert any(most[p] != 0 and has_row(p, 0) and KEYS * outside_end_runs(p) < row for p in range(positions))  # a row the end runs cover
        assert any(0 < total[p, 0] and not has_row(p, 0) for p in range(positions))  # '-' as escape keys
        if name == "block":
            shares = total[list(CODE_PLANES)] / N
            assert ((shares > 0.15).sum(axis=1) == 6).all()
        if name == "long":
            assert (is_missing[:, 1_023] & is_missing[:, 1_024]).sum() >= len(MISSING_ROWS) + 60  # runs across the finish blocks' border
            crafted = {position for s, position, *_ in CRAFTED if s == LONG}
            stretch = sym[:, QUIET[0]:QUIET[1]]
            keyed = symbols.is_valid[stretch] & (stretch != data.dominant[store][None, QUIET[0]:QUIET[1]])
            for position in range(*QUIET):
                if position not in crafted:
                    column = keyed[:, position - QUIET[0]]
                    assert column[:131_072].sum() == 2 and column[131_072:].sum() == 2, position
    for store, position, filter_name, proportion, one_more in CRAFTED:
        bound, symbol = data.bounds[store][position]
        want = data.want[store][filter_name]
        assert want[position, symbols.scan_index(symbol)] == bound + (1 if one_more else 0)
        assert sa.must_exceed(want[position].sum(), proportion) == bound  # the selection's own threshold at the position
        assert position not in data.never_pruned[store]


def test_the_stores_derive_symbols_and_the_long_one_has_overflow_keys(store, data):
    for k in range(3):
        assert store.scan_runs(k) > 0       # derived symbols, X kept as runs
        assert store.scan_escapes(k) > 0
        covered, events, _ = store.scan_end_runs(k)
        print(GENES[k][0], "covered rows", covered, "end events", events, "overflow keys", store.scan_overflow_keys(k))
    assert store.scan_end_runs(BLOCK)[0] > 0 and store.scan_end_runs(LONG)[0] > 0
    assert store.scan_rows(BLOCK, CODE_PLANES[0], CODE_PLANES[-1] + 1) > 12  # code planes, not one-hot rows
    assert store.scan_overflow_keys(LONG) > 0   # the quiet stretch
    assert store.scan_overflow_keys(SHORT) == 0  # 75 codons are 1 650 counters: every key fits its granule
    cardinality = int(data.masks["random 40 %"].sum())
    for k in (BLOCK, LONG):  # something to leave out at 0.05 under the 40 % filter: granules of keys and one-hot rows
        skippable, total = store.scan_prunable_granules(k, cardinality, 0.05)
        assert 0 < skippable <= total, (k, skippable, total)
        skippable, total = store.scan_prunable_rows(k, cardinality, 0.05)
        assert 0 < skippable <= total, (k, skippable, total)


# ---- the exact scan ------------------------------------------------------------------------------------------------------------------
# the three stores, and sub-ranges that begin and end inside runs of X, inside the quiet stretch and on either side of the finish
# blocks' border
RANGES = WHOLE + [(LONG, 150, 1_250), (LONG, 300, 900), (LONG, 1_023, 1_300), (LONG, 0, 1_024), (LONG, 1_024, 1_025), (LONG, 1_025, 1_300),
                  (LONG, 640, 641), (BLOCK, 1, 1_023), (SHORT, 3, 70)]


def check_exact(store, data, names, settings):
    gap_events, end_runs = settings.get(sa.TUNE_GAP_EVENTS, 0), settings.get(sa.TUNE_END_RUNS, 0)
    tables, kernels = sa.timed(store, settings, lambda: store.mutations_scan_ranges(RANGES, [store.filters[name] for name in names]))
    if settings.get(sa.TUNE_SIDE_STREAM, 0) == 3:  # neither gap events nor slice-major keys
        assert not any(k.startswith("k_scan_escapes_sliced<") for k in kernels), kernels
        assert any(k.startswith("k_scan_missing_runs") for k in kernels) and "k_finish_scan<false, 0>" in kernels, kernels
    else:
        sa.check_kernels(kernels, len(names), gap_events, end_runs)
    for (k, a, b), per_filter in zip(RANGES, tables):
        for name, table in zip(names, per_filter):
            assert np.array_equal(table, data.want[k][name][a:b]), (settings, GENES[k][0], a, b, name)


@pytest.mark.parametrize("q_count", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("gap_events, end_runs", [(0, 0), (0, 1), (0, -1), (-1, 0)])
def test_exact_tables_of_three_stores_in_one_call(store, data, q_count, gap_events, end_runs):
    check_exact(store, data, FILTERS[:q_count], {sa.TUNE_GAP_EVENTS: gap_events, sa.TUNE_END_RUNS: end_runs})


@pytest.mark.parametrize("side_stream", [2, 3])
def test_exact_tables_with_every_pass_on_one_stream(store, data, side_stream):
    check_exact(store, data, FILTERS[:4], {sa.TUNE_SIDE_STREAM: side_stream})


def test_batch_entry_over_a_sub_range(store, data):
    tables = store.mutations_scan_batch(LONG, [store.filters[name] for name in FILTERS], 150, 1_250)
    for name, table in zip(FILTERS, tables):
        assert np.array_equal(table, data.want[LONG][name][150:1_250]), name


# ---- the pruning entry ---------------------------------------------------------------------------------------------------------------
def pruned_scan(store, names, proportions, knob=0, ranges=WHOLE):
    (tables, kernels) = sa.timed(store, {sa.TUNE_PRUNE_KEYS: knob},
                                 lambda: store.mutations_scan_ranges(ranges, [store.filters[name] for name in names], min_proportions=proportions))
    return tables, kernels


def check_pruned_tables(store, data, tables, names, proportions, label):
    for k, per_filter in enumerate(tables):
        for name, proportion, pruned in zip(names, proportions, per_filter):
            sa.check_pruned(store, pruned, data.want[k][name], data.reference_index[k], proportion, data.never_pruned[k], (label, GENES[k][0], name))


@pytest.mark.parametrize("proportion", PROPORTIONS)
def test_pruned_tables_keep_row_sums_and_selected_rows(store, data, proportion):
    for knob in (0, 1, -1):  # keys and rows left out; keys only; nothing
        for names in (["random 40 %"], ["all rows"], FILTERS) if knob == 0 else (["random 40 %"], ["all rows"]):
            tables, kernels = pruned_scan(store, names, [proportion] * len(names), knob)
            assert any(", pruning" in k for k in kernels) == (knob >= 0 and proportion > 0), kernels
            check_pruned_tables(store, data, tables, names, [proportion] * len(names), (knob, proportion))
            exact = all(np.array_equal(pruned, data.want[k][name]) for k, per_filter in enumerate(tables) for name, pruned in zip(names, per_filter))
            if knob < 0 or proportion == 0:
                assert exact
            elif len(names) == 1 and proportion in (0.05, 0.5):  # (the knob made a difference: something was left out)
                assert not exact


def test_groups_on_the_bound_and_one_above(store, data):
    """A group of exactly must_exceed rows is not reported, a group of one more is, with its exact count — in `block` as keys
    (all rows at 0.01) and as one-hot rows (the 40 % filter at 0.05), in `long` inside the quiet stretch, where the keys that
    decide lie on the overflow list."""
    symbols = data.symbols
    for filter_name, proportion in (("all rows", 0.01), ("random 40 %", 0.05)):
        for knob in (0, 1):
            tables, _ = pruned_scan(store, [filter_name], [proportion], knob)
            for k, position, crafted_filter, crafted_proportion, one_more in CRAFTED:
                if (crafted_filter, crafted_proportion) != (filter_name, proportion):
                    continue
                bound, symbol = data.bounds[k][position]
                index = symbols.scan_index(symbol)
                pruned, want = tables[k][0], data.want[k][filter_name]
                rows = sa.selected_rows(store, pruned, data.reference_index[k], proportion)
                if one_more:
                    assert pruned[position, index] == bound + 1
                    assert (position, index, bound + 1, int(want[position].sum())) in rows
                else:
                    assert want[position, index] == bound
                    assert not any(row[0] == position and row[1] == index for row in rows)


def test_eight_filters_with_their_own_proportions(store, data):
    proportions = [0.05, 0.01, 0.05, 0.0, 0.5, 1.0, 0.01, 0.5]
    tables, kernels = pruned_scan(store, FILTERS, proportions)
    assert any(", pruning" in k for k in kernels), kernels
    check_pruned_tables(store, data, tables, FILTERS, proportions, "own proportions")
    ranges = [(LONG, 150, 1_250), (LONG, 1_024, 1_300), (BLOCK, 1, 1_023)]
    names = ["random 40 %", "all rows", "random 90 %"]
    for proportion in (0.01, 0.05):
        tables, _ = pruned_scan(store, names, [proportion] * 3, ranges=ranges)
        for (k, a, b), per_filter in zip(ranges, tables):
            never = [p - a for p in data.never_pruned[k] if a <= p < b]
            for name, pruned in zip(names, per_filter):
                sa.check_pruned(store, pruned, data.want[k][name][a:b], data.reference_index[k][a:b], proportion, never, (GENES[k][0], a, b, name))


# ---- the scan that selects its rows ------------------------------------------------------------------------------------------------
CAPACITY = 65_536  # more than the 21 x 2 399 cells a proportion of 0 can select


@pytest.fixture(scope="module")
def sinks(store, data):
    from silo_amd import binding

    made = Built()
    made.reference_index = np.concatenate(data.reference_index)
    reference = np.ascontiguousarray(made.reference_index)
    made.reference_dev = ctypes.c_void_p()
    assert store.lib.silo_gpu_upload_bytes(reference.ctypes.data_as(ctypes.c_void_p), reference.nbytes, ctypes.byref(made.reference_dev)) == 0
    made.slots = [binding.RowSlot(CAPACITY) for _ in FILTERS]
    made.tables = [store.malloc(4 * TOTAL_POSITIONS * 22) for _ in FILTERS]
    made.exact = {name: table_of([data.want[k][name] for k in range(3)]) for name in FILTERS}
    yield made
    for slot in made.slots:
        slot.close()
    store.lib.silo_gpu_free(made.reference_dev)


def scan_select(store, sinks, names, proportions, knob, ranges=WHOLE, offsets=TABLE_OFFSET, slots=None):
    """One call of silo_gpu_mutations_scan_select into tables filled with 0xA5: ([(table, n_selected, sorted rows)] per filter, kernels)."""
    slots = slots or sinks.slots[:len(names)]
    tables = sinks.tables[:len(names)]
    for table in tables:
        store.memset(table, 0xA5, 4 * TOTAL_POSITIONS * 22)
    _, kernels = sa.timed(store, {sa.TUNE_FUSED_SELECT: knob}, lambda: store.mutations_scan_select(
        list(ranges), [store.filters[name] for name in names], proportions, tables, list(offsets), TOTAL_POSITIONS, sinks.reference_dev, slots))
    out = []
    for table, slot in zip(tables, slots):
        n_selected, rows = slot.wait()
        out.append((store.read(table, np.uint32, TOTAL_POSITIONS * 22).reshape(TOTAL_POSITIONS, 22), n_selected, sorted(map(tuple, rows.tolist()))))
    return out, kernels


@pytest.mark.parametrize("names", [FILTERS[:1], [FILTERS[0], FILTERS[3]], FILTERS], ids=["1 filter", "2 filters", "8 filters"])
@pytest.mark.parametrize("proportion", PROPORTIONS)
def test_selected_rows_and_tables_of_the_finish_kernel(store, data, sinks, names, proportion):
    proportions = [proportion] * len(names)
    pruned = store.mutations_scan_ranges(WHOLE, [store.filters[name] for name in names], min_proportions=proportions)
    for knob in (0, -1):
        results, kernels = scan_select(store, sinks, names, proportions, knob)
        # 0: the finish kernel of 22 symbols stores the tables and selects — no fill, no selection launch; -1: the call clears, scans and selects
        assert ("k_finish_scan<true, 22>" in kernels) == (knob == 0) and ("k_finish_scan<true, 0>" in kernels) == (knob < 0), kernels
        for q, (name, (table, n_selected, rows)) in enumerate(zip(names, results)):
            exact = sinks.exact[name]
            want_rows = sa.oracle_rows(exact, sinks.reference_index, proportion)
            assert n_selected == len(rows) == len(want_rows), (knob, name)
            assert rows == want_rows, (knob, name)
            assert np.array_equal(table.sum(axis=1, dtype=np.uint32), exact.sum(axis=1, dtype=np.uint32)), (knob, name)
            assert np.array_equal(table, table_of([pruned[k][q] for k in range(3)])), (knob, name)  # whatever it held before
            if proportion == 0:
                assert np.array_equal(table, exact), (knob, name)
        if proportion in (0.01, 0.05):  # (not vacuous: the crafted groups of one more row are among the rows)
            for k, position, filter_name, crafted_proportion, one_more in CRAFTED:
                if one_more and crafted_proportion == proportion and filter_name in names:
                    bound, symbol = data.bounds[k][position]
                    row = (TABLE_OFFSET[k] + position, data.symbols.scan_index(symbol), bound + 1)
                    assert row in {r[:3] for r in results[names.index(filter_name)][2]}


def test_ranges_that_do_not_tile_the_table(store, data, sinks):
    """A sub-range of `long`: the call clears the table, scans and launches the selection; the same rows."""
    a, b = 100, 1_200
    for proportion in (0.0, 0.05):
        results, kernels = scan_select(store, sinks, FILTERS[:1], [proportion], 0, ranges=[(LONG, a, b)], offsets=[TABLE_OFFSET[LONG] + a])
        assert "k_finish_scan<true, 0>" in kernels and "k_finish_scan<true, 22>" not in kernels, kernels
        (table, n_selected, rows), = results
        exact = np.zeros_like(sinks.exact[FILTERS[0]])
        exact[TABLE_OFFSET[LONG] + a:TABLE_OFFSET[LONG] + b] = data.want[LONG][FILTERS[0]][a:b]
        want_rows = sa.oracle_rows(exact, sinks.reference_index, proportion)
        assert (n_selected, rows) == (len(want_rows), want_rows)
        assert np.array_equal(table.sum(axis=1, dtype=np.uint32), exact.sum(axis=1, dtype=np.uint32))
        assert not table[:TABLE_OFFSET[LONG] + a].any() and not table[TABLE_OFFSET[LONG] + b:].any()


def test_more_rows_than_the_slot_holds(store, data, sinks):
    from silo_amd import binding

    small = binding.RowSlot(4)
    try:
        results, kernels = scan_select(store, sinks, FILTERS[:1], [0.0], 0, slots=[small])
        assert "k_finish_scan<true, 22>" in kernels, kernels
        (table, n_selected, rows), = results
        want_rows = sa.oracle_rows(sinks.exact[FILTERS[0]], sinks.reference_index, 0.0)
        assert n_selected == len(want_rows) > 4  # the header carries the true count
        assert len(rows) == 4 and set(rows) <= set(want_rows)
        assert np.array_equal(table, sinks.exact[FILTERS[0]])  # complete for the caller's fallback
    finally:
        small.close()
