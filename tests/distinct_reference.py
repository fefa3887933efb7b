"""The numpy statement of DistinctSequences (K20): a 128-bit hash of every row of a symbol matrix and one row per class of rows.

    splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                   z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31                                 (mod 2^64)
    x = position * 32 + symbol;   H0(position, symbol) = splitmix64(x);   H1(position, symbol) = splitmix64(x + 2^40)
    hash(row) = (sum over positions of H0(p, sym[row, p]), sum over positions of H1(p, sym[row, p]))         (mod 2^64 each)

sym[row, p] is the index of the row's symbol at p in the alphabet's own order, NO_SYMBOL (31) for a cell without one.  Rows are
GLOBAL row numbers.  Of every class of selected rows — equal rows, or rows with equal hashes — the representative is the one with
the smallest number; the selection is the set of representatives."""
import numpy as np

NO_SYMBOL = 31
LANE_OFFSET = 1 << 40


def splitmix64(z):
    """splitmix64 of an array of uint64 (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def terms(positions, symbols, lane):
    """H0 (lane 0) / H1 (lane 1) of cells given as arrays of positions and symbols, as uint64."""
    x = np.asarray(positions, dtype=np.uint64) * np.uint64(32) + np.asarray(symbols, dtype=np.uint64)
    return splitmix64(x + np.uint64(LANE_OFFSET if lane else 0))


def row_hashes(sym):
    """uint64 [rows][2]: the hash of every row of a symbol matrix [rows][positions]."""
    sym = np.asarray(sym)
    out = np.zeros((sym.shape[0], 2), dtype=np.uint64)
    positions = np.arange(sym.shape[1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for lane in (0, 1):
            out[:, lane] = terms(positions[None, :], sym, lane).sum(axis=1, dtype=np.uint64)
    return out


def _first_of_each_class(rows, class_of_row):
    """bool over all rows: of the rows `rows` (ascending) the first one of every class."""
    _, first = np.unique(class_of_row, return_index=True)
    return rows[first]


def select_by_hash(hashes, selected):
    """bool [rows]: of the selected rows the one with the smallest number of every class of equal hashes (uint64 [rows][2])."""
    selected = np.asarray(selected, dtype=bool)
    rows = np.flatnonzero(selected)
    out = np.zeros(len(selected), dtype=bool)
    if len(rows):
        _, class_of_row = np.unique(np.asarray(hashes, dtype=np.uint64)[rows], axis=0, return_inverse=True)
        out[_first_of_each_class(rows, class_of_row.reshape(-1))] = True
    return out


def select_by_equality(sym, selected):
    """The same by exact equality of the rows of a symbol matrix."""
    selected = np.asarray(selected, dtype=bool)
    rows = np.flatnonzero(selected)
    out = np.zeros(len(selected), dtype=bool)
    if len(rows):
        _, class_of_row = np.unique(np.asarray(sym)[rows], axis=0, return_inverse=True)
        out[_first_of_each_class(rows, class_of_row.reshape(-1))] = True
    return out


def select(sym, selected):
    """The representatives of a symbol matrix under a selection — by hash, checked against exact equality: a fixture with a
    collision (there is none to be expected in 2^128) would fail here, on the CPU."""
    by_hash = select_by_hash(row_hashes(sym), selected)
    assert np.array_equal(by_hash, select_by_equality(sym, selected))
    return by_hash


def symbols_of_strings(strings, chars, missing, length):
    """The symbol matrix of aligned sequences given as strings over the alphabet `chars` ('.' reads as '-', 'U' as 'T' among
    nucleotides, as the store does); None — a row without a sequence — is the missing symbol throughout."""
    table = np.full(256, 255, dtype=np.uint8)
    for index, char in enumerate(chars):
        table[ord(char)] = index
    if chars.startswith("-ACGT"):
        table[ord(".")] = 0
        table[ord("U")] = 4
    sym = np.full((len(strings), length), chars.index(missing), dtype=np.uint8)
    for row, text in enumerate(strings):
        if text is not None:
            sym[row] = table[np.frombuffer(text.encode(), dtype=np.uint8)]
    assert (sym != 255).all()
    return sym
