"""The numpy statement of K22 (CellCount / CellCountDistribution): the four cell counts of every row of a symbol matrix against a
reference, the value a kinds mask sums, the rows a pair of bounds selects and the bins of a histogram.

sym[row, p] and reference[p] are indices in the alphabet's own order ("-ACGTRYSWKMBDHVN" / "-ACDEFGHIKLMNPQRSTVWYBZ*X"), NO_SYMBOL
(31) for a cell without one.  The class of a cell is K18's (tests/sequence_differences_reference.py), on indices: MISSING where the
symbol is N / X whatever the reference holds; AMBIGUOUS where it is any other symbol that is no valid mutation symbol; SAME where it
is valid and the reference's; DELETION where it is valid, differs and is '-'; SUBSTITUTION otherwise.  cells(row) counts them in the
order substitutions, deletions, missing, ambiguous."""
import numpy as np

NUC = "-ACGTRYSWKMBDHVN"
AA = "-ACDEFGHIKLMNPQRSTVWYBZ*X"
CHARS = {"nuc": NUC, "aa": AA}
VALID = {"nuc": "-ACGT", "aa": "-ACDEFGHIKLMNPQRSTVWY*"}
MISSING_SYMBOL = {"nuc": NUC.index("N"), "aa": AA.index("X")}
NO_SYMBOL = 31
KINDS = ("substitutions", "deletions", "missing", "ambiguous")
SUBSTITUTIONS, DELETIONS, MISSING, AMBIGUOUS = 1, 2, 4, 8
MAX_BINS = 4096


def mask_of(kinds):
    """The kinds mask of a kind or a list of kinds."""
    kinds = [kinds] if isinstance(kinds, str) else list(kinds)
    assert kinds and len(set(kinds)) == len(kinds)
    return sum(1 << KINDS.index(kind) for kind in kinds)


def cells(sym, reference, alphabet):
    """uint32 [rows][4]: the cell counts of every row of sym [rows][P] against reference [P]."""
    sym = np.asarray(sym)
    reference = np.asarray(reference)
    valid = np.zeros(256, dtype=bool)
    valid[[CHARS[alphabet].index(c) for c in VALID[alphabet]]] = True
    is_missing = sym == MISSING_SYMBOL[alphabet]
    is_ambiguous = ~valid[sym] & ~is_missing
    differs = valid[sym] & (sym != reference[None, :])
    is_deletion = differs & (sym == 0)
    is_substitution = differs & (sym != 0)
    return np.stack([kind.sum(axis=1) for kind in (is_substitution, is_deletion, is_missing, is_ambiguous)], axis=1).astype(np.uint32).reshape(-1, 4)


def values(table, kinds_mask):
    """uint64 [rows]: the sum of the kinds of kinds_mask of a table uint32 [rows][4]."""
    table = np.asarray(table, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(len(table), dtype=np.uint64)
    for k in range(4):
        if (kinds_mask >> k) & 1:
            out += table[:, k]
    return out


def selected(table, n, kinds_mask, at_least=0, at_most=0xFFFFFFFF):
    """bool [rows of the table]: row < n and at_least <= value <= at_most."""
    value = values(table, kinds_mask)
    return (np.arange(len(value)) < n) & (value >= np.uint64(at_least)) & (value <= np.uint64(at_most))


def bins(table, rows, kinds_mask, bin_width, n_bins):
    """uint64 [n_bins]: the rows `rows` (bool over the table's rows) by min(value / bin_width, n_bins - 1)."""
    value = values(table, kinds_mask)[np.asarray(rows, dtype=bool)]
    index = np.minimum(value // np.uint64(bin_width), np.uint64(n_bins - 1)).astype(np.int64)
    return np.bincount(index, minlength=n_bins).astype(np.uint64)


def response_rows(histogram, bin_width):
    """The rows of a CellCountDistribution response for the bins uint64 [maxBins]."""
    last = len(histogram) - 1
    return [{"from": b * bin_width, "to": None if b == last else b * bin_width + bin_width - 1, "count": int(histogram[b])}
            for b in range(len(histogram)) if histogram[b]]


def symbols_of_chars(chars, alphabet):
    """The symbol indices of characters uint8 [...] as silo_gpu_reconstruct_sequences writes them ('?' is NO_SYMBOL)."""
    table = np.full(256, 255, dtype=np.uint8)
    table[np.frombuffer(CHARS[alphabet].encode(), dtype=np.uint8)] = np.arange(len(CHARS[alphabet]), dtype=np.uint8)
    table[ord("?")] = NO_SYMBOL
    sym = table[np.asarray(chars, dtype=np.uint8)]
    assert (sym != 255).all()
    return sym
