"""The numpy reference of the comparison of count tables (K17, silo_gpu_mutations_compare) and of the rows that MutationsComparison /
AminoAcidMutationsComparison make of it — test infrastructure only.

Pinned against a plain loop over positions, symbols and groups and against hand-made rows by
tests/test_mutations_comparison_reference.py and used by tests/test_mutations_compare_gpu.py and tests/test_mutations_comparison_gpu.py.
"""
import numpy as np

from tests.consensus_reference import VALID, count_table, reference_index_of

MAX_TABLES = 64     # SILO_GPU_MAX_COMPARISON_TABLES
THREADS = 256       # SILO_GPU_COMPARE_THREADS: the positions that a block of K17 owns
HEADER_WORDS = 4    # of the output of silo_gpu_mutations_compare: word 0 is the number of selected cells
FIRST_CAPACITY = 1024  # the records the first call of a MutationsComparison request has room for


def compare_tables(tables, reference_index, min_proportion, min_difference):
    """For tables uint32 [T][P][n_symbols] and reference_index uint8 [P] (0xFF: none): (records uint32 [K][2] = (position, symbol),
    ascending; cells uint32 [K][T][2] = (count, coverage) of every table; difference float64 [K]; passes bool [K][T]) of the K selected
    cells.  Table t passes (p, s) iff its coverage cov (the sum of the position's counts) is above 0 and the count is above
    0 if min_proportion == 0 else uint32(ceil(float64(cov) * min_proportion) - 1); difference = the highest minus the lowest float64
    count / cov over the covered tables (0.0 without one); selected iff s is not the reference's, some table passes and difference >=
    min_difference."""
    tables = np.asarray(tables, dtype=np.uint32)
    n_tables, positions, n_symbols = tables.shape
    reference_index = np.asarray(reference_index, dtype=np.uint8)
    assert reference_index.shape == (positions,) and 0 <= min_proportion <= 1 and 0 <= min_difference <= 1
    wide = tables.astype(np.uint64)
    coverage = wide.sum(axis=-1)  # [T][P]
    assert coverage.max(initial=0) <= 0xFFFFFFFF
    covered = coverage > 0
    if min_proportion == 0:
        bound = np.zeros_like(coverage)
    else:
        bound = np.where(covered, np.ceil(coverage.astype(np.float64) * np.float64(min_proportion)) - 1, 0).astype(np.uint64)
    passes = covered[..., None] & (wide > bound[..., None])  # [T][P][S]
    with np.errstate(divide="ignore", invalid="ignore"):
        proportion = wide.astype(np.float64) / coverage.astype(np.float64)[..., None]
    highest = np.where(covered[..., None], proportion, -np.inf).max(axis=0)
    lowest = np.where(covered[..., None], proportion, np.inf).min(axis=0)
    difference = np.where(covered.any(axis=0)[:, None], highest - lowest, 0.0)  # [P][S]
    not_reference = np.arange(n_symbols)[None, :] != reference_index[:, None]
    selected = not_reference & passes.any(axis=0) & (difference >= np.float64(min_difference))
    at = np.argwhere(selected)  # ascending by (position, symbol)
    p, s = at[:, 0], at[:, 1]
    cells = np.stack([tables[:, p, s].T, np.broadcast_to(coverage[:, p].T, (len(p), n_tables)).astype(np.uint32)], axis=-1).astype(np.uint32)
    return at.astype(np.uint32), cells.reshape(len(p), n_tables, 2), difference[p, s], passes[:, p, s].T.reshape(len(p), n_tables)


def comparison_rows(tables, reference_chars, alphabet, sequence_name, group_names, min_proportion=0.05, min_difference=0.0):
    """The rows of a response, in the order position, symbol, group: for tables uint32 [G][P][n_symbols] of the groups `group_names`
    and the reference sequence's characters."""
    records, cells, difference, _ = compare_tables(tables, reference_index_of(reference_chars, alphabet), min_proportion, min_difference)
    rows = []
    for (position, symbol), of_groups, spread in zip(records.tolist(), cells.tolist(), difference.tolist()):
        mutation = f"{reference_chars[position]}{position + 1}{VALID[alphabet][symbol]}"
        for name, (count, coverage) in zip(group_names, of_groups):
            rows.append({"mutation": mutation, "sequenceName": sequence_name, "position": position + 1, "group": name, "count": count, "coverage": coverage,
                         "proportion": float(np.float64(count) / np.float64(coverage)) if coverage else None, "difference": spread})
    return rows


def group_tables(chars_of_groups, alphabet, positions):
    """uint32 [G][P][n_symbols]: the Mutations table of every group's characters uint8 [n][P] (n may be 0)."""
    return np.stack([count_table(np.asarray(chars, dtype=np.uint8).reshape(-1, positions), alphabet) for chars in chars_of_groups])


def unpack(out, n_tables, capacity):
    """(selected, records uint32 [fit][2], cells uint32 [fit][T][2]) of the words silo_gpu_mutations_compare leaves, the records put in
    ascending order with their cells; fit = min(selected, capacity)."""
    out = np.asarray(out, dtype=np.uint32)
    selected = int(out[0])
    fit = min(selected, capacity)
    records = out[HEADER_WORDS:HEADER_WORDS + 2 * fit].reshape(fit, 2)
    begin = HEADER_WORDS + 2 * capacity
    cells = out[begin:begin + fit * n_tables * 2].reshape(fit, n_tables, 2)
    order = np.lexsort((records[:, 1], records[:, 0]))
    return selected, records[order], cells[order]


# Rows worked out by hand, nucleotides "-ACGT": (what it is about, the counts of one position in every table, the reference's symbol
# index, minProportion, minDifference, {selected symbol: its difference}).
HAND_MADE = [
    ("at K4's bound: ceil(100 * 0.05) - 1 = 4 < 5", [[0, 95, 5, 0, 0], [0, 100, 0, 0, 0]], 1, 0.05, 0.0, {2: 0.05}),
    ("one below the bound in both tables", [[0, 96, 4, 0, 0], [0, 96, 4, 0, 0]], 1, 0.05, 0.0, {}),
    ("below the bound in one table, at it in the other", [[0, 96, 4, 0, 0], [0, 95, 5, 0, 0]], 1, 0.05, 0.0, {2: 0.05 - 0.04}),
    ("minProportion 0: a count of 1 passes, a count of 0 never", [[0, 9, 1, 0, 0], [0, 10, 0, 0, 0]], 1, 0.0, 0.0, {2: 0.1}),
    ("minProportion 1: the whole coverage", [[0, 0, 7, 0, 0], [0, 6, 1, 0, 0]], 1, 1.0, 0.0, {2: 1 - 1 / 7}),
    ("minProportion 1: nobody holds the whole coverage", [[0, 1, 6, 0, 0], [0, 6, 1, 0, 0]], 1, 1.0, 0.0, {}),
    ("one table covered: the difference is 0.0", [[0, 2, 8, 0, 0], [0, 0, 0, 0, 0]], 1, 0.05, 0.0, {2: 0.0}),
    ("one table covered, a minDifference above 0", [[0, 2, 8, 0, 0], [0, 0, 0, 0, 0]], 1, 0.05, 0.01, {}),
    ("no table covered", [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], 1, 0.0, 0.0, {}),
    ("1/4 against 3/4: the difference is minDifference exactly", [[0, 3, 1, 0, 0], [0, 1, 3, 0, 0]], 1, 0.05, 0.5, {2: 0.5}),
    ("1/4 against 3/4, minDifference the next double", [[0, 3, 1, 0, 0], [0, 1, 3, 0, 0]], 1, 0.05, float(np.nextafter(0.5, 1.0)), {}),
    ("the reference's symbol differs most: never a row", [[0, 10, 0, 0, 0], [0, 0, 9, 1, 0]], 1, 0.05, 0.0, {2: 0.9, 3: 0.1}),
    ("the reference's symbol differs most, minDifference 0.5", [[0, 10, 0, 0, 0], [0, 0, 9, 1, 0]], 1, 0.05, 0.5, {2: 0.9}),
    ("no reference symbol (0xFF): every symbol is eligible", [[0, 10, 0, 0, 0], [0, 0, 9, 1, 0]], 0xFF, 0.05, 0.0, {1: 1.0, 2: 0.9, 3: 0.1}),
    ("identical tables: the difference is 0.0", [[1, 5, 3, 0, 1], [1, 5, 3, 0, 1]], 1, 0.05, 0.0, {0: 0.0, 2: 0.0, 4: 0.0}),
    ("identical tables, a minDifference above 0", [[1, 5, 3, 0, 1], [1, 5, 3, 0, 1]], 1, 0.05, 0.01, {}),
    ("the highest count a cell can hold", [[0, 0, 2**32 - 1, 0, 0], [0, 1, 0, 0, 0]], 1, 0.5, 1.0, {2: 1.0}),
    ("three tables: the middle one neither highest nor lowest", [[0, 8, 2, 0, 0], [0, 5, 5, 0, 0], [0, 1, 9, 0, 0]], 1, 0.5, 0.7, {2: 0.9 - 0.2}),
]
