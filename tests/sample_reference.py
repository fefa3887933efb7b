"""The numpy statement of Sample (K19): a keyed permutation of the database's row numbers and the rows with the smallest keys.

    fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16                       (mod 2^32)
    splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                   z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31                                 (mod 2^64)
    k = splitmix64(seed); k1, k2 = its low and high 32 bits;   key(seed, row) = fmix32(fmix32(row + k1) ^ k2)

Every step is a bijection of uint32, so two rows never share a key.  Rows are GLOBAL row numbers: a row's number in the database,
whatever partition holds it.  Without groups the selection is the min(size, |C|) rows of C with the smallest keys; with groups the
union over the groups of the min(size, |C_g|) rows of C_g with the smallest keys, rows of C in no group (NO_GROUP) never."""
import numpy as np

NO_GROUP = 0xFFFF
MASK64 = (1 << 64) - 1


def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def splitmix64(z):
    z = (int(z) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def keys(seed, rows):
    """key(seed, row) for an array of global row numbers, as uint32."""
    k = splitmix64(seed)
    rows = np.asarray(rows, dtype=np.uint32)
    with np.errstate(over="ignore"):
        return fmix32(fmix32(rows + np.uint32(k & 0xFFFFFFFF)) ^ np.uint32(k >> 32))


def select(seed, size, selected, groups=None, first_row=0):
    """The rows Sample selects, as a bool array like `selected` (bool per row; row i is the global row first_row + i).  groups:
    None, or a group per row (NO_GROUP: none)."""
    selected = np.asarray(selected, dtype=bool)
    row_keys = keys(seed, np.arange(len(selected), dtype=np.uint64) + first_row)
    out = np.zeros(len(selected), dtype=bool)
    if groups is None:
        strata = [np.flatnonzero(selected)]
    else:
        groups = np.asarray(groups)
        strata = [np.flatnonzero(selected & (groups == group)) for group in np.unique(groups[selected & (groups != NO_GROUP)])]
    for rows in strata:
        out[rows[np.argsort(row_keys[rows], kind="stable")[:size]]] = True
    return out


def date_groups(selected, dates, range_bounds):
    """The date range (index into range_bounds, uint32 [n][2] = from, to, both inclusive) of every selected row as uint16, NO_GROUP
    for a row that is not selected, whose date is NULL (0) or that lies in no range."""
    selected = np.asarray(selected, dtype=bool)
    dates = np.asarray(dates, dtype=np.uint64)
    out = np.full(len(selected), NO_GROUP, dtype=np.uint16)
    for index, (date_from, date_to) in enumerate(np.asarray(range_bounds, dtype=np.uint64).reshape(-1, 2)):
        out[selected & (dates != 0) & (dates >= date_from) & (dates <= date_to)] = index
    return out


def words(mask, row_words=None):
    """A bool per row as uint64 row-bitset words (row_words of them: zero padding behind the rows)."""
    mask = np.asarray(mask, dtype=bool)
    n_words = (len(mask) + 63) // 64 if row_words is None else row_words
    padded = np.zeros(n_words * 64, dtype=bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)
