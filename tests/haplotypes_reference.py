"""A plain numpy reference of Haplotypes / AminoAcidHaplotypes (K16) over a symbol matrix uint8 [rows][positions]
of symbol ids: the symbol columns silo_gpu_position_symbols writes, the tuple ids and the row bitset of silo_gpu_haplotype_ids, and
the response rows of the action.  Pinned without a GPU by tests/test_haplotypes_reference.py.
"""
from collections import Counter

import numpy as np

SYMBOL_NONE = 0xFF
MAX_POSITIONS = 12
POSITIONS_PER_COLUMN = 6
ALL_COMPLETE = 0xFFFFFFFF


def padded_rows(n):
    """Rows of a store's columns: whole 256-byte lines of the row bitsets (2 048 rows), at least one."""
    return max(1, (n + 2047) // 2048) * 2048


def position_symbols(sym, positions, rows=None):
    """uint8 [len(positions)][rows]: the symbol id of every row at the listed positions (0-based, repeats allowed), SYMBOL_NONE
    for the rows past the matrix."""
    sym = np.asarray(sym, dtype=np.uint8)
    rows = padded_rows(len(sym)) if rows is None else rows
    out = np.full((len(positions), rows), SYMBOL_NONE, dtype=np.uint8)
    out[:, :len(sym)] = sym[:, list(positions)].T
    return out


def mask_of(symbols):
    """complete_symbols: bit s for every symbol id of `symbols`."""
    return int(sum(1 << int(s) for s in symbols))


def _in_mask(symbols, complete_symbols):
    """Per byte: is it in the mask?  A byte of 32 or more is no bit of it: in only where the mask leaves nothing out."""
    symbols = symbols.astype(np.int64)
    low = (np.int64(complete_symbols) >> np.minimum(symbols, 31)) & 1
    return np.where(symbols < 32, low != 0, complete_symbols == ALL_COMPLETE)


def haplotype_ids(symbols, sequence_count, n_symbols):
    """uint32 [ceil(k / 6)][rows]: column j of row r is sum_i symbols[6 j + i][r] * n_symbols^(m - 1 - i), the first position most
    significant; 0 in every column for a row with a byte at or past n_symbols and for the rows at or past sequence_count."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    k, rows = symbols.shape
    n_columns = (k + POSITIONS_PER_COLUMN - 1) // POSITIONS_PER_COLUMN
    known = (symbols < n_symbols).all(axis=0) & (np.arange(rows) < sequence_count)
    out = np.zeros((n_columns, rows), dtype=np.uint64)
    for j in range(n_columns):
        for c in range(POSITIONS_PER_COLUMN * j, min(k, POSITIONS_PER_COLUMN * (j + 1))):
            out[j] = out[j] * np.uint64(n_symbols) + symbols[c]
    out[:, ~known] = 0
    assert int(out.max(initial=0)) < 2**32
    return out.astype(np.uint32)


def complete_rows(symbols, sequence_count, complete_symbols=ALL_COMPLETE, filter_words=None):
    """uint64 [rows / 64]: bit r = r < sequence_count && filter bit r (None: every row) && every listed symbol of r is in the mask."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    rows = symbols.shape[1]
    selected = _in_mask(symbols, complete_symbols).all(axis=0) & (np.arange(rows) < sequence_count)
    if filter_words is not None:
        bits = np.unpackbits(np.ascontiguousarray(filter_words, dtype="<u8").view(np.uint8), bitorder="little")[:rows]
        selected &= bits.astype(bool)
    return np.packbits(selected, bitorder="little").view("<u8").astype(np.uint64)


def haplotype_rows(sym, positions, chars, mask=None, valid_symbols=None, groups=None):
    """The response rows of the action over the matrix: positions 0-based in request order, chars the alphabet (index = symbol id),
    mask the selected rows (None: all), valid_symbols the ids a row must hold at every listed position (excludeIncomplete; None:
    every row counts), groups a list of per-row tuples of group values (None: no groupByFields).  A list of dicts {"groups":
    tuple, "haplotype": str, "count": int, "proportion": float}, sorted by (groups as text, haplotype)."""
    sym = np.asarray(sym, dtype=np.uint8)
    columns = sym[:, list(positions)]
    selected = np.ones(len(sym), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    if valid_symbols is not None:
        selected &= np.isin(columns, list(valid_symbols)).all(axis=1)
    table = np.frombuffer(chars.encode("ascii") if isinstance(chars, str) else bytes(chars), dtype=np.uint8)
    taken = np.nonzero(selected)[0]
    k = columns.shape[1]
    # the distinct haplotypes of the selected rows as byte strings (no character of an alphabet is NUL), and which one a row has
    letters = np.ascontiguousarray(table[columns[taken]]).view(f"S{k}").reshape(-1)
    distinct, which = (np.unique(letters, return_inverse=True) if len(taken) else (np.zeros(0, f"S{k}"), np.zeros(0, np.int64)))
    keys = [() if groups is None else tuple(groups[row]) for row in taken.tolist()]
    counter = Counter(zip(keys, which.reshape(-1).tolist()))
    counter = {(key, distinct[index].decode("ascii")): count for (key, index), count in counter.items()}
    total = sum(counter.values())
    rows = [dict(groups=key, haplotype=haplotype, count=count, proportion=count / total) for (key, haplotype), count in counter.items()]
    rows.sort(key=lambda row: (tuple(str(v) for v in row["groups"]), row["haplotype"]))
    return rows
