"""The numpy statement of DistinctSequenceCounts (K21) on top of tests/distinct_reference.py: the classes of a selection as
{representative: count} — the representative is the class's smallest selected GLOBAL row, the count its number of selected rows —
by equal hashes and by exact equality of the rows of a symbol matrix, and the keys the device packs them into:

    key(count, row) = (0xFFFFFFFF - count) << 32 | row

so that ascending keys are descending counts, then ascending representatives."""
import numpy as np

from tests import distinct_reference as ref


def _classes(rows, class_of_row, first_row):
    """{representative: count} of the rows `rows` (ascending) with the class number of each."""
    _, first, counts = np.unique(class_of_row, return_index=True, return_counts=True)
    return {int(rows[f]) + first_row: int(c) for f, c in zip(first, counts)}


def classes_by_hash(hashes, selected, first_row=0):
    """The classes of equal hashes (uint64 [rows][2]) among the selected rows; row r is the global row first_row + r."""
    rows = np.flatnonzero(np.asarray(selected, dtype=bool))
    if not len(rows):
        return {}
    _, class_of_row = np.unique(np.asarray(hashes, dtype=np.uint64)[rows], axis=0, return_inverse=True)
    return _classes(rows, class_of_row.reshape(-1), first_row)


def classes_by_equality(sym, selected, first_row=0):
    """The same by exact equality of the rows of a symbol matrix."""
    rows = np.flatnonzero(np.asarray(selected, dtype=bool))
    if not len(rows):
        return {}
    _, class_of_row = np.unique(np.asarray(sym)[rows], axis=0, return_inverse=True)
    return _classes(rows, class_of_row.reshape(-1), first_row)


def classes(sym, selected):
    """The classes of a symbol matrix under a selection — by hash, checked against exact equality (a fixture with a collision would
    fail here, on the CPU)."""
    by_hash = classes_by_hash(ref.row_hashes(sym), selected)
    assert by_hash == classes_by_equality(sym, selected)
    return by_hash


def key(count, row):
    return ((0xFFFFFFFF - int(count)) << 32) | int(row)


def packed_keys(class_counts, min_count=1):
    """uint64, ascending: the keys of the classes of at least min_count rows."""
    return np.array(sorted(key(count, row) for row, count in class_counts.items() if count >= min_count), dtype=np.uint64)


def first_keys(class_counts, k, min_count=1):
    """The first k of them: the classes an answer lists, in its order."""
    return packed_keys(class_counts, min_count)[:k]


def unpack(keys):
    """[(count, row)] of an array of keys, in its order."""
    return [(0xFFFFFFFF - (int(k) >> 32), int(k) & 0xFFFFFFFF) for k in keys]
