"""The numpy reference of K18 (silo_gpu_sequence_differences) and of the rows of MutationsPerSequence / AminoAcidMutationsPerSequence:
the class of every cell of a matrix of characters against a reference, the record words of the rows with their offsets and four cell
counts, and the response's lists and counts of a row.  numpy only; tests/test_sequence_differences_reference.py pins it against a
plain loop over rows and positions.

The rule (include/silo_gpu.h, K18).  With "valid" the mutation symbols of the alphabet and the missing symbol N / X, a cell with the
byte c at position p is MISSING if c is the missing symbol; AMBIGUOUS if c is any other byte that is not valid; SAME if c is valid and
the reference's byte at p; DELETION if c is valid, differs and is '-'; SUBSTITUTION otherwise.  It emits the word (p << 9) | (close <<
8) | byte iff it is a SUBSTITUTION or AMBIGUOUS (byte = c); or a DELETION or MISSING whose left neighbour IN THE SAME ROW has another
class or does not exist (a run start, byte = c); or SAME with a left neighbour that is a DELETION or MISSING (a close: byte = 0,
close = 1)."""
import numpy as np

VALID = {"nuc": "-ACGT", "aa": "-ACDEFGHIKLMNPQRSTVWY*"}
MISSING_SYMBOL = {"nuc": "N", "aa": "X"}
SAME, SUBSTITUTION, DELETION, MISSING, AMBIGUOUS = range(5)
STATS = 4                   # substitution, deleted, missing, ambiguous cells of a row
MAX_ROWS = 10_000
MAX_POSITIONS = 1 << 23
CHUNK = 4096                # bytes of a row per block of K18: 256 threads x 16 bytes, from the 16-byte boundary at or below the row
QUAD = 16                   # bytes per thread
WAVE_BYTES = 64 * QUAD      # bytes per wave
FIRST_WORDS_PER_ROW = 32    # the action's first capacity is this many words per selected row
LIST_FIELDS = ("substitutions", "deletions", "missing", "ambiguous")
COUNT_FIELDS = ("substitutionCount", "deletedPositions", "missingPositions", "ambiguousPositions")


def _bytes(text_or_array):
    if isinstance(text_or_array, (str, bytes)):
        raw = text_or_array.encode("latin-1") if isinstance(text_or_array, str) else text_or_array
        return np.frombuffer(raw, dtype=np.uint8)
    return np.asarray(text_or_array, dtype=np.uint8)


def classify(chars, reference, alphabet):
    """uint8 [n][P]: the class of every cell of chars uint8 [n][P] against reference (P bytes or a string)."""
    chars = np.asarray(chars, dtype=np.uint8)
    reference = _bytes(reference)
    valid = np.zeros(256, dtype=bool)
    valid[_bytes(VALID[alphabet])] = True
    classes = np.full(chars.shape, SUBSTITUTION, dtype=np.uint8)
    classes[chars == ord("-")] = DELETION
    classes[chars == reference[None, :]] = SAME
    classes[~valid[chars]] = AMBIGUOUS
    classes[chars == ord(MISSING_SYMBOL[alphabet])] = MISSING
    return classes


def difference_records(chars, reference, alphabet):
    """(offsets uint32 [n + 1], stats uint32 [n][4], words uint32 [offsets[n]]): what silo_gpu_sequence_differences writes with a
    capacity of at least offsets[n]."""
    chars = np.asarray(chars, dtype=np.uint8)
    n, positions = chars.shape
    classes = classify(chars, reference, alphabet)
    left = np.full((n, positions), 0xFF, dtype=np.uint8)  # left of position 0: no class at all
    left[:, 1:] = classes[:, :-1]
    run = (classes == DELETION) | (classes == MISSING)
    close = (classes == SAME) & ((left == DELETION) | (left == MISSING))
    emits = (classes == SUBSTITUTION) | (classes == AMBIGUOUS) | (run & (left != classes)) | close
    rows, at = np.nonzero(emits)  # row-major: by row, then by ascending position
    words = (at.astype(np.uint32) << np.uint32(9)) | np.where(close[rows, at], np.uint32(0x100), chars[rows, at].astype(np.uint32))
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(emits.sum(axis=1, dtype=np.int64))
    stats = np.stack([(classes == k).sum(axis=1) for k in (SUBSTITUTION, DELETION, MISSING, AMBIGUOUS)], axis=1).astype(np.uint32).reshape(n, STATS)
    return offsets, stats, words.astype(np.uint32)


def _runs(flags):
    """'a-b,c': the maximal runs of set flags, 1-based and inclusive."""
    padded = np.concatenate([[False], flags, [False]]).astype(np.int8)
    edges = np.flatnonzero(np.diff(padded))
    return ",".join(str(first + 1) if past - first == 1 else f"{first + 1}-{past}" for first, past in zip(edges[::2].tolist(), edges[1::2].tolist()))


def row_fields(chars_row, reference, alphabet):
    """The eight fields of a response row that derive from the sequence: the four lists as comma-joined strings ("" when empty) and
    the four counts.  The caller adds the primary key and sequenceName."""
    row = np.asarray(chars_row, dtype=np.uint8)
    reference = _bytes(reference)
    classes = classify(row[None, :], reference, alphabet)[0]

    def named(cell_class):
        return ",".join(chr(reference[p]) + str(p + 1) + chr(row[p]) for p in np.flatnonzero(classes == cell_class).tolist())

    lists = (named(SUBSTITUTION), _runs(classes == DELETION), _runs(classes == MISSING), named(AMBIGUOUS))
    fields = dict(zip(LIST_FIELDS, lists))
    for field, cell_class in zip(COUNT_FIELDS, (SUBSTITUTION, DELETION, MISSING, AMBIGUOUS)):
        fields[field] = int((classes == cell_class).sum())
    return fields


def response_rows(keys, chars, reference, alphabet, sequence_name, key_field):
    """The response of the action for the rows `chars` with the primary keys `keys`, in that order."""
    return [dict(row_fields(chars[r], reference, alphabet), **{key_field: keys[r], "sequenceName": sequence_name}) for r in range(len(keys))]


def _reference_text(alphabet, length, offset=0):
    symbols = VALID[alphabet][1:]  # no '-' in a reference
    return "".join(symbols[(p + offset) % len(symbols)] for p in range(length))


def _hand_made():
    """(what, alphabet, reference, rows, the words expected of each row as (position, close, byte)) — worked out by hand."""
    n, x = ord("N"), ord("X")
    cases = [
        ("a row equal to the reference", "nuc", "ACGTACGT", ["ACGTACGT"], [[]]),
        ("a row that is all N", "nuc", "ACGTACGT", ["NNNNNNNN"], [[(0, 0, n)]]),
        ("a run that starts at position 0", "nuc", "ACGTACGT", ["--GTACGT"], [[(0, 0, 45), (2, 1, 0)]]),
        ("a run that ends at the last position", "nuc", "ACGTACGT", ["ACGTACNN"], [[(6, 0, n)]]),
        ("a close at the last position", "nuc", "ACGTACGT", ["ACGTA--T"], [[(5, 0, 45), (7, 1, 0)]]),
        ("a one-cell run", "nuc", "ACGTACGT", ["ACGNACGT"], [[(3, 0, n), (4, 1, 0)]]),
        ("a deletion run directly followed by a missing run, and the reverse", "nuc", "ACGTACGT", ["A--NNCGT", "ANN--CGT"],
         [[(1, 0, 45), (3, 0, n), (5, 1, 0)], [(1, 0, n), (3, 0, 45), (5, 1, 0)]]),
        ("a run followed by a substitution", "nuc", "ACGTACGT", ["A--AACGT"], [[(1, 0, 45), (3, 0, 65)]]),
        ("a run followed by an ambiguous cell", "nuc", "ACGTACGT", ["ANNRACGT"], [[(1, 0, n), (3, 0, 82)]]),
        ("two adjacent substitutions", "nuc", "ACGTACGT", ["ACTGACGT"], [[(2, 0, 84), (3, 0, 71)]]),
        ("a row that ends in an N run, then a row that begins with N", "nuc", "ACGTACGT", ["ACGTACNN", "NNGTACGT"],
         [[(6, 0, n)], [(0, 0, n), (2, 1, 0)]]),
        ("a row that ends in a deletion run, then a row that begins with one", "nuc", "ACGTACGT", ["ACGTAC--", "--GTACGT"],
         [[(6, 0, 45)], [(0, 0, 45), (2, 1, 0)]]),
        ("a row that ends in a run, then a row that begins like the reference: no close", "nuc", "ACGTACGT", ["ACGTAC--", "ACGTACGT"],
         [[(6, 0, 45)], []]),
        ("the bytes 0x00, 0xFF and a are ambiguous", "nuc", "ACGTACGT", [b"A\x00GT\xffCaT"], [[(1, 0, 0), (4, 0, 255), (6, 0, 97)]]),
        ("a 0x00 byte after a run is no close", "nuc", "ACGTACGT", [b"AN\x00TACGT"], [[(1, 0, n), (2, 0, 0)]]),
        ("a reference that holds N and a lower-case letter", "nuc", "ANgTACGT", ["ANGTACGT", "ACgTACGT", "A-GTACGT"],
         [[(1, 0, n), (2, 0, 71)], [(1, 0, 67), (2, 0, 103)], [(1, 0, 45), (2, 0, 71)]]),
        ("amino acids: N is valid, X is missing, B is ambiguous, * is valid", "aa", "MNK*LX", ["MNK*LX", "MXK-LA", "MBN*-X"],
         [[(5, 0, x)], [(1, 0, x), (2, 1, 0), (3, 0, 45), (4, 1, 0), (5, 0, 65)], [(1, 0, 66), (2, 0, 78), (4, 0, 45), (5, 0, x)]]),
    ]
    return cases


HAND_MADE = _hand_made()


def hand_made_matrix(case):
    """(chars uint8 [n][P], reference uint8 [P], words as difference_records orders them) of a HAND_MADE case."""
    _, _, reference, rows, expected = case
    chars = np.stack([_bytes(row) for row in rows])
    words = [(p << 9) | (close << 8) | byte for of_row in expected for p, close, byte in of_row]
    return chars, _bytes(reference), np.array(words, dtype=np.uint32)


def skewed_chars(rng, alphabet, n, positions, reference=None):
    """(chars uint8 [n][P], reference uint8 [P]): rows that mostly equal the reference, with substitutions, runs of '-' and of the
    missing symbol of every length (at the ends of rows too, so that a row ends in a run and the next begins with one), ambiguity
    codes, and a few bytes that are no symbol at all."""
    reference = _bytes(_reference_text(alphabet, positions, int(rng.integers(0, 4))) if reference is None else reference).copy()
    chars = np.repeat(reference[None, :], n, axis=0).copy()
    symbols = _bytes(VALID[alphabet])
    cells = rng.random((n, positions))
    chars[cells < 0.03] = symbols[rng.integers(0, len(symbols), size=int((cells < 0.03).sum()))]
    codes = _bytes("RYKMSWBDHVryacgt" if alphabet == "nuc" else "BZJOUbzx")
    chars[cells > 0.99] = codes[rng.integers(0, len(codes), size=int((cells > 0.99).sum()))]
    chars[(cells > 0.985) & (cells < 0.987)] = 0x00
    chars[(cells > 0.987) & (cells < 0.989)] = 0xFF
    missing = ord(MISSING_SYMBOL[alphabet])
    for row in range(n):
        for _ in range(int(rng.integers(0, 4))):
            length = int(rng.choice([1, 2, 3, 17, 70, 300, positions]))
            start = int(rng.integers(-length // 2, positions))
            chars[row, max(start, 0):start + length] = missing if rng.random() < 0.6 else ord("-")
        if rng.random() < 0.3:
            chars[row, -int(rng.integers(1, 4)):] = missing if rng.random() < 0.5 else ord("-")
        if rng.random() < 0.3:
            chars[row, :int(rng.integers(1, 4))] = missing if rng.random() < 0.5 else ord("-")
    for row, symbol in ((0, missing), (2, ord("-"))):  # for certain: a row that ends in a run, and the next begins with one of its kind
        if row + 1 < n:
            chars[row, -2:] = symbol
            chars[row + 1, :2] = symbol
    return chars, reference
