"""Naive per-character checker over a symbol matrix — test infrastructure only.

The second, representation-free oracle of SURVEY.md §7 step 1: it never builds a bitmap index, it
counts characters.  Used to pin both the reference-shaped oracle (oracle/silo_oracle.py) and the HIP
kernels on the same inputs.
"""
import numpy as np


def pack_bits(mask):
    """bool [N] -> uint64 words, bit i of word w = row 64*w + i (little endian)."""
    mask = np.asarray(mask, dtype=bool)
    n_words = (len(mask) + 63) // 64
    padded = np.zeros(n_words * 64, dtype=bool)
    padded[: len(mask)] = mask
    return np.packbits(padded, bitorder="little").view("<u8").copy()


def unpack_bits(words, n):
    words = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def plane(symbols, position, symbol):
    """Membership set C[p][s] of SURVEY.md §3.6 as packed words."""
    return pack_bits(symbols[:, position] == symbol)


def mutation_counts(symbols, filter_mask, scan_symbols, pos_begin=0, pos_end=None):
    """uint32 [positions][len(scan_symbols)]: |F ∧ C[p][s]| by direct counting (mutations.cpp:64-164)."""
    symbols = np.asarray(symbols)
    if pos_end is None:
        pos_end = symbols.shape[1]
    selected = symbols[np.asarray(filter_mask, dtype=bool), pos_begin:pos_end]
    out = np.zeros((pos_end - pos_begin, len(scan_symbols)), dtype=np.uint32)
    for k, s in enumerate(scan_symbols):
        out[:, k] = (selected == s).sum(axis=0, dtype=np.int64)
    return out


NO_GROUP = 0xFFFF


def row_groups(mask, dates, ranges):
    """uint16 [N]: the index in `ranges` (inclusive (from, to) pairs, pairwise disjoint, in request order) of the range a
    selected row's date lies in, NO_GROUP for rows outside the mask, rows with a NULL date (0) and rows in no range."""
    mask = np.asarray(mask, dtype=bool)
    dates = np.asarray(dates, dtype=np.int64)
    groups = np.full(len(mask), NO_GROUP, dtype=np.uint16)
    for g, (low, high) in enumerate(ranges):
        groups[mask & (dates != 0) & (dates >= int(low)) & (dates <= int(high))] = g
    return groups


def grouped_mutation_counts(symbols, mask, dates, ranges, cells, scan_symbols):
    """uint32 [len(cells)][len(ranges)][2] for cells = (position, symbol) pairs: per range the rows of the mask whose date
    lies in it (from <= date <= to, date != 0) that carry the symbol at the position (count), and those that carry any of
    scan_symbols there (coverage)."""
    symbols = np.asarray(symbols)
    mask = np.asarray(mask, dtype=bool)
    dates = np.asarray(dates, dtype=np.int64)
    valid = np.zeros(256, dtype=bool)
    valid[np.asarray(list(scan_symbols), dtype=np.int64)] = True
    out = np.zeros((len(cells), len(ranges), 2), dtype=np.uint32)
    for g, (low, high) in enumerate(ranges):
        rows = np.nonzero(mask & (dates != 0) & (dates >= int(low)) & (dates <= int(high)))[0]
        if len(rows) == 0:
            continue
        columns = {}
        for m, (position, symbol) in enumerate(cells):
            position = int(position)
            if position not in columns:
                columns[position] = symbols[rows, position]
            column = columns[position]
            out[m, g, 0] = np.count_nonzero(column == symbol)
            out[m, g, 1] = np.count_nonzero(valid[column])
    return out
