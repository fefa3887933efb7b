"""Alignments for the tests of the Mutations scan over stores with derived symbols, for either alphabet: the generators and checks
that tests/test_gap_events_gpu.py, test_end_runs_gpu.py, test_pruned_scan_gpu.py, test_pruned_rows_gpu.py and
test_fused_select_gpu.py each carry for nucleotides, driven by silo_amd.alphabet.  A plain module: it builds no store and asks no
device by itself."""
import contextlib
import math

import numpy as np

from oracle import dense

GAP = 0  # '-' in both alphabets: a valid mutation symbol, and what an alignment's ragged ends are made of
TUNE_SIDE_STREAM, TUNE_SCAN_TIMING, TUNE_LAUNCH_COST, TUNE_GAP_EVENTS, TUNE_PRUNE_KEYS, TUNE_END_RUNS, TUNE_FUSED_SELECT = 5, 7, 9, 10, 11, 12, 13
KEY_COST_BYTES = 10  # layout_choice.h: a symbol of a position gets a one-hot row once its keys would cost more than the row
NO_REFERENCE = 255   # the reference index of a position whose reference symbol is no scan symbol


class Symbols:
    """What a generator needs of an alphabet ('nuc' or 'aa'): the valid mutation symbols in scan order, the missing symbol, the
    ambiguity codes (every other symbol) and the character of every symbol id."""

    def __init__(self, name):
        from silo_amd import alphabet

        table = alphabet.ALPHABETS[name]
        self.name = name
        self.count = table.count
        self.valid = np.array(table.valid_mutation_symbols, dtype=np.uint8)
        self.letters = self.valid[self.valid != GAP]  # the valid symbols a settled position is made of
        self.missing = int(table.missing)
        self.ambiguity = np.array([s for s in range(table.count) if s not in set(self.valid.tolist()) and s != table.missing], dtype=np.uint8)
        self.chars = np.frombuffer(table.chars.encode(), dtype=np.uint8)
        self.n_scan = len(self.valid)
        self.is_valid = np.zeros(256, dtype=bool)
        self.is_valid[self.valid] = True

    def scan_index(self, symbol):
        return int(np.flatnonzero(self.valid == symbol)[0])

    def symbol(self, char):
        return int(np.flatnonzero(self.chars == ord(char))[0])


def row_bytes(n_rows):
    """Bytes of a plane row of a store of n_rows sequences (rows are padded to 32 words)."""
    return (n_rows + 2047) // 2048 * 256


def settled_positions(rng, symbols, n, dominant, second, third, second_share=0.002, third_share=0.0002, other_share=0.001):
    """uint8 [n][len(dominant)]: per position one valid symbol in nearly every row, a second one in `second_share` of them (a number
    or one per position), a third in `third_share`, and the symbols that are not valid — the missing symbol, the ambiguity codes —
    in `other_share`.  Generated in chunks of positions."""
    positions = len(dominant)
    second_share = np.broadcast_to(np.asarray(second_share, dtype=np.float32), (positions,))
    third_share = np.broadcast_to(np.asarray(third_share, dtype=np.float32), (positions,))
    others = np.r_[symbols.ambiguity, symbols.missing].astype(np.uint8)
    sym = np.empty((n, positions), dtype=np.uint8)
    for a in range(0, positions, 256):
        b = min(a + 256, positions)
        draw = rng.random((n, b - a), dtype=np.float32)
        two, three = second_share[None, a:b], second_share[None, a:b] + third_share[None, a:b]
        chunk = np.where(draw < two, second[None, a:b], dominant[None, a:b]).astype(np.uint8)
        chunk = np.where((draw >= two) & (draw < three), third[None, a:b], chunk)
        lone = draw >= np.float32(1.0 - other_share)
        chunk[lone] = others[rng.integers(0, len(others), size=int(lone.sum()))]
        sym[:, a:b] = chunk
    return sym


def symbol_orders(rng, symbols, positions):
    """(dominant, second, third) [positions]: three different letters (valid symbols other than the gap symbol) per position."""
    orders = np.array([rng.permutation(symbols.letters)[:3] for _ in range(positions)], dtype=np.uint8)
    return orders[:, 0].copy(), orders[:, 1].copy(), orders[:, 2].copy()


def add_missing_runs(rng, symbols, sym, rows, mean, crossing=()):
    """Runs of the missing symbol of geometric length (mean `mean`) in the given rows — one to three each, every seventh row's
    first from position 0 — with an ambiguity code right behind or right in front of some; then, per (from, to, count) of
    `crossing`, `count` more of the rows get a run that starts in the `from` interval and ends in the `to` interval."""
    positions = sym.shape[1]
    for k, row in enumerate(rows):
        for _ in range(1 + k % 3):
            start = 0 if k % 7 == 0 else int(rng.integers(0, positions))
            end = min(positions, start + int(rng.geometric(1 / mean)))
            sym[row, start:end] = symbols.missing
            if k % 5 == 0 and end < positions:
                sym[row, end] = rng.choice(symbols.ambiguity)
            if k % 5 == 1 and start > 0:
                sym[row, start - 1] = rng.choice(symbols.ambiguity)
    at = 0
    for (from_low, from_high), (to_low, to_high), count in crossing:
        for row in rows[at:at + count]:
            sym[row, int(rng.integers(from_low, from_high)):int(rng.integers(to_low, to_high))] = symbols.missing
        at += count


def add_lone_codes(rng, symbols, sym, rows, count):
    """`count` cells, in the given rows, get an ambiguity code."""
    cells_r = rng.choice(rows, size=count)
    cells_p = rng.integers(0, sym.shape[1], size=count)
    sym[cells_r, cells_p] = symbols.ambiguity[rng.integers(0, len(symbols.ambiguity), size=count)]


def add_ragged_ends(rng, sym, rows, lead_mean, trail_mean, longest):
    """Leading and trailing runs of the gap symbol of geometric length, at most `longest` positions, in the given rows; returns
    (lead, trail) [len(rows)]."""
    positions = sym.shape[1]
    lead = np.minimum(rng.geometric(1 / lead_mean, size=len(rows)), longest)
    trail = np.minimum(rng.geometric(1 / trail_mean, size=len(rows)), longest)
    for row, head, tail in zip(rows, lead, trail):
        sym[row, :head] = GAP
        sym[row, positions - tail:] = GAP
    return lead, trail


def end_runs_of(sym):
    """(lead, trail_start) [n] as the store defines them: the first position that is not the gap symbol, and the position behind
    the last one; both the number of positions for a row of the gap symbol throughout."""
    positions = sym.shape[1]
    not_gap = sym != GAP
    some = not_gap.any(axis=1)
    lead = np.where(some, not_gap.argmax(axis=1), positions)
    trail_start = np.where(some, positions - not_gap[:, ::-1].argmax(axis=1), positions)
    return lead, trail_start


def craft_group(symbols, sym, position, dominant, symbol, eligible, size):
    """Position `position` becomes `dominant` in every row that has a letter there (the gap symbol and the symbols that are not
    valid stay), then `symbol` in the first `size` of the `eligible` rows that have a letter there.  Returns the group's rows."""
    column = sym[:, position]
    letter = symbols.is_valid[column] & (column != GAP)
    column[letter] = dominant
    group = eligible[letter[eligible]][:size]
    assert len(group) == size
    column[group] = symbol
    return group


# ---- filters: unions of disjoint classes of rows, so that the oracle counts every row once ---------------------------------------
class RowClasses:
    """The rows of a store in disjoint classes (a label per row).  A filter is a set of labels; the oracle's table of a filter is
    the sum of dense.mutation_counts over its classes — counts are additive over rows —, so the oracle reads every row once however
    many filters there are."""

    def __init__(self, labels):
        self.labels = np.asarray(labels)
        self.classes = np.unique(self.labels)
        self.filters = {}  # name: (labels of the filter, mask)

    def add(self, name, chosen):
        chosen = [label for label in self.classes if chosen(label)]
        self.filters[name] = (chosen, np.isin(self.labels, chosen))

    def mask(self, name):
        return self.filters[name][1]

    def names(self):
        return list(self.filters)

    def oracle_tables(self, sym, scan_symbols, first_row=0):
        """{name: dense.mutation_counts(sym, the filter's rows)} for the rows [first_row, first_row + len(sym)) of the store."""
        labels = self.labels[first_row:first_row + len(sym)]
        per_class = {label: dense.mutation_counts(sym, labels == label, scan_symbols) for label in self.classes if (labels == label).any()}
        zero = np.zeros((sym.shape[1], len(scan_symbols)), dtype=np.uint32)
        return {name: sum((per_class[label] for label in chosen if label in per_class), zero.copy()) for name, (chosen, _) in self.filters.items()}


def upload(store, masks):
    pointers = []
    for mask in masks:
        pointers.append(store.bitset_alloc())
        store.bitset_upload(pointers[-1], dense.pack_bits(mask))
    return pointers


@contextlib.contextmanager
def tuned(store, settings):
    """The knobs of `settings` ({knob: value}) set for the block and put back behind it."""
    previous = []
    try:
        for knob, value in settings.items():
            previous.append((knob, store.tune(knob, value)))
        yield
    finally:
        for knob, value in reversed(previous):
            store.tune(knob, value)


def timed(store, settings, call):
    """(call(), the kernel names of the scan's timing log) with the knobs of `settings` set."""
    from silo_amd import binding

    with tuned(store, {**settings, TUNE_SCAN_TIMING: 1}):
        result = call()
        kernels = [entry["kernel"] for entry in binding.scan_timings()]
    return result, kernels


def check_kernels(kernels, q_count, gap_events, end_runs):
    """The launches of a scan of a store with derived symbols, gap events and end runs under SILO_GPU_TUNE_GAP_EVENTS = gap_events
    and SILO_GPU_TUNE_END_RUNS = end_runs."""
    escapes = [k for k in kernels if k.startswith("k_scan_escapes_sliced<")]
    per_block = 1 if q_count <= 1 else (2 if q_count <= 2 else (4 if q_count <= 4 else 8))
    assert escapes and all(k.startswith("k_scan_escapes_sliced<%u>" % per_block) for k in escapes), kernels
    separate = [k for k in kernels if k.startswith(("k_scan_missing_runs", "k_count_sparse_keys"))]
    if gap_events < 0:  # the runs and the sparse keys by themselves, no end runs
        assert any(k.startswith("k_scan_missing_runs") for k in separate), kernels
        assert not any(", ends" in k for k in kernels), kernels
        assert "k_finish_scan<false, 0>" in kernels, kernels
        return
    assert not separate, kernels
    assert "k_finish_scan<true, 0>" in kernels, kernels
    if end_runs < 0:
        assert not any(", ends" in k for k in kernels), kernels
    elif end_runs == 0:
        assert any(", ends" in k for k in escapes), kernels
    else:  # the end events in a launch of their own behind the others
        assert ", ends" not in escapes[0] and ", ends" in escapes[-1] and len(escapes) >= 2, kernels


# ---- the pruning contract (silo_gpu_mutations_scan_ranges_min_proportion) and the row selection (K4) -------------------------------
def must_exceed(covered, proportion):
    return int(math.ceil(float(covered) * proportion) - 1)


def reference_index(scan_symbols, reference):
    scan_symbols = list(scan_symbols)
    return np.array([scan_symbols.index(s) if s in scan_symbols else NO_REFERENCE for s in reference], dtype=np.uint8)


def selected_rows(store, table, reference, proportion):
    n, rows = store.mutations_select(table, reference, proportion, capacity=table.size)
    assert n == len(rows)
    return sorted(map(tuple, rows.tolist()))


def oracle_rows(table, reference, proportion):
    """The row selection of K4 (silo_gpu.h) over an exact table, in numpy: sorted (position, symbol, count, total)."""
    covered = table.sum(axis=1, dtype=np.uint32)
    bound = np.zeros(len(table), dtype=np.uint32)
    if proportion != 0:
        positive = covered > 0
        bound[positive] = (np.ceil(covered[positive].astype(np.float64) * proportion) - 1).astype(np.uint32)
    passes = (table > bound[:, None]) & (covered[:, None] > 0)
    passes[np.arange(len(table))[reference != NO_REFERENCE], reference[reference != NO_REFERENCE]] = False
    return sorted((int(p), int(s), int(table[p, s]), int(covered[p])) for p, s in zip(*np.nonzero(passes)))


def check_pruned(store, pruned, exact, reference, proportion, never_pruned=(), label=""):
    """What a pruned table owes: every position's row sum, the rows the selection reports from it — with the store's reference
    symbols and that proportion —, and every cell of a position that derives another symbol than the reference's, or none
    (`never_pruned`: such positions, relative to the table's first)."""
    assert np.array_equal(pruned.sum(axis=1, dtype=np.uint32), exact.sum(axis=1, dtype=np.uint32)), (label, proportion)
    want = oracle_rows(exact, reference, proportion)
    assert selected_rows(store, pruned, reference, proportion) == selected_rows(store, exact, reference, proportion) == want, (label, proportion)
    never_pruned = np.asarray(list(never_pruned), dtype=np.int64)
    assert np.array_equal(pruned[never_pruned], exact[never_pruned]), (label, proportion)
    if proportion == 0:
        assert np.array_equal(pruned, exact), label
