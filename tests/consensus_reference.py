"""The numpy reference of the consensus call (K15, silo_gpu_consensus_call) — test infrastructure only.

Pinned against a plain character double loop and hand-made rows by tests/test_consensus_reference.py and used by
tests/test_consensus_call_gpu.py and tests/test_consensus_gpu.py.
"""
import numpy as np

from tests.pair_distances_reference import AA_VALID, NOT_VALID, NUC_VALID, code_table

MAX_TABLES = 64     # SILO_GPU_MAX_CONSENSUS_TABLES
THREADS = 256       # SILO_GPU_CONSENSUS_THREADS: positions of one table that a block of K15 owns
VALID = {"nuc": NUC_VALID, "aa": AA_VALID}
MISSING = {"nuc": "N", "aa": "X"}
# the sets of ACGT (bit k: the k-th of them) as the characters of a call
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "AC": "M", "AG": "R", "AT": "W", "CG": "S", "CT": "Y", "GT": "K", "ACG": "V", "ACT": "H",
         "AGT": "D", "CGT": "B", "ACGT": "N"}
# every character a call can be
CALL_CHARS = {"nuc": "-ACGTMRWSYKVHDBN", "aa": AA_VALID + "X"}
AMBIGUOUS, LOW_COVERAGE, DELETED, DIFFERENCES = range(4)  # the words of a summary


def _nucleotide_table():
    """uint8 [32]: the character of a set of "-ACGT" (bit s: symbol s) of one or more symbols."""
    table = np.zeros(32, dtype=np.uint8)
    for mask in range(1, 32):
        members = "".join(NUC_VALID[s] for s in range(5) if mask >> s & 1)
        if members == "-":
            table[mask] = ord("-")
        elif "-" in members:
            table[mask] = ord("N")
        else:
            table[mask] = ord(IUPAC[members])
    return table


def call_consensus(counts, reference_index, alphabet, threshold, min_depth):
    """(chars uint8 [...][P], summary uint32 [...][4]) for counts uint32 [...][P][n_symbols] — any number of tables in front — and
    reference_index uint8 [P] (0xFF: the reference symbol is not a valid one): what silo_gpu_consensus_call leaves.  depth = sum of a
    position's counts; below min_depth the missing symbol; otherwise need = ceil(float64(depth) * threshold) and the call is every
    symbol whose count is at least that of the symbol at which the descending counts first sum to need."""
    counts = np.asarray(counts, dtype=np.uint32)
    valid = VALID[alphabet]
    assert counts.shape[-1] == len(valid) and 0 < threshold <= 1 and min_depth >= 1
    positions = counts.shape[-2]
    reference_index = np.asarray(reference_index, dtype=np.uint8)
    assert reference_index.shape == (positions,)
    wide = counts.astype(np.uint64)
    depth = wide.sum(axis=-1)
    assert depth.max(initial=0) <= 0xFFFFFFFF
    low = depth < min_depth
    need = np.ceil(depth.astype(np.float64) * np.float64(threshold)).astype(np.uint64)
    descending = -np.sort(-wide.astype(np.int64), axis=-1)
    reached = np.cumsum(descending, axis=-1).astype(np.uint64) >= need[..., None]
    cut = np.take_along_axis(descending, reached.argmax(axis=-1)[..., None], axis=-1).astype(np.uint64)
    taken = (wide >= cut) & ~low[..., None]  # (cut > 0 wherever depth > 0)
    size = taken.sum(axis=-1)
    first = taken.argmax(axis=-1)
    ambiguous = size > 1
    if alphabet == "nuc":
        masks = (taken << np.arange(5)).sum(axis=-1)
        chars = _nucleotide_table()[masks]
    else:
        chars = np.where(ambiguous, ord("X"), np.frombuffer(valid.encode(), dtype=np.uint8)[first]).astype(np.uint8)
    chars = np.where(low, ord(MISSING[alphabet]), chars).astype(np.uint8)
    single = ~low & ~ambiguous
    deleted = single & (first == 0)
    differs = single & (first != reference_index)
    summary = np.stack([ambiguous.sum(axis=-1), low.sum(axis=-1), deleted.sum(axis=-1), differs.sum(axis=-1)], axis=-1).astype(np.uint32)
    return chars, summary


def count_table(chars, alphabet):
    """uint32 [P][n_symbols] for chars uint8 [n][P]: per position the rows that hold each valid symbol — a Mutations table."""
    chars = np.asarray(chars, dtype=np.uint8)
    codes = code_table(VALID[alphabet])[chars]
    return np.stack([(codes == s).sum(axis=0) for s in range(len(VALID[alphabet]))], axis=-1).astype(np.uint32)


def reference_index_of(reference_chars, alphabet):
    """uint8 [P]: the index of every reference character among the valid symbols, 0xFF where it is none of them."""
    return code_table(VALID[alphabet])[np.frombuffer(reference_chars.encode("latin-1"), dtype=np.uint8)]


def consensus_row(chars, reference_chars, alphabet, threshold=0.5, min_depth=1):
    """The fields of a response row that come off the device, for the characters uint8 [n][P] of a group's rows."""
    chars = np.asarray(chars, dtype=np.uint8).reshape(-1, len(reference_chars))
    called, summary = call_consensus(count_table(chars, alphabet), reference_index_of(reference_chars, alphabet), alphabet, threshold, min_depth)
    return {
        "count": int(chars.shape[0]), "consensus": called.tobytes().decode("latin-1"), "ambiguousPositions": int(summary[AMBIGUOUS]),
        "lowCoveragePositions": int(summary[LOW_COVERAGE]), "deletedPositions": int(summary[DELETED]), "differences": int(summary[DIFFERENCES]),
    }


assert NOT_VALID == 0xFF


def _nuc(gap=0, a=0, c=0, g=0, t=0):
    return [gap, a, c, g, t]


def _aa(**counts):
    row = [0] * len(AA_VALID)
    for name, count in counts.items():
        row[AA_VALID.index({"gap": "-", "stop": "*"}.get(name, name))] = count
    return row


# Rows worked out by hand: (alphabet, the counts of one position, threshold, minDepth, the call, what the position is — "single",
# "ambiguous", "low" or "deleted").  need = ceil(depth * threshold) is in the comment where it decides.
HAND_MADE = [("nuc", _nuc(**{m.lower(): 7 for m in members}), 1.0, 1, code, "ambiguous" if len(members) > 1 else "single") for members, code in IUPAC.items()] + [
    ("nuc", _nuc(gap=5, a=5), 0.75, 1, "N", "ambiguous"),         # need 8: both, and '-' is one of them
    ("nuc", _nuc(gap=10), 0.5, 1, "-", "deleted"),
    ("nuc", _nuc(gap=6, a=3, c=1), 0.5, 1, "-", "deleted"),       # need 5
    ("nuc", _nuc(a=4, c=4, t=1), 0.4, 1, "M", "ambiguous"),       # need 4: one symbol reaches it, its tie comes along
    ("nuc", _nuc(a=4, c=4, t=1), 0.5, 1, "M", "ambiguous"),       # need 5
    ("nuc", _nuc(a=3, c=3, g=3, t=1), 0.3, 1, "V", "ambiguous"),  # need 3: a three-way tie
    ("nuc", _nuc(2, 2, 2, 2, 2), 0.1, 1, "N", "ambiguous"),       # need 1: a five-way tie, '-' among them
    ("nuc", _nuc(a=2, c=2, g=2, t=2), 1e-9, 1, "N", "ambiguous"),  # need 1: ACGT
    ("nuc", _nuc(a=5, c=3, g=1), 0.85, 1, "M", "ambiguous"),      # need 8 == 5 + 3
    ("nuc", _nuc(a=5, c=3, g=1), 0.9, 1, "V", "ambiguous"),       # need 9 == 5 + 3 + 1: the two stop at need - 1
    ("nuc", _nuc(a=6, c=2, t=2), 0.9, 1, "H", "ambiguous"),       # need 9: 6 is short, the tied pair goes in whole
    ("nuc", _nuc(), 0.5, 1, "N", "low"),                          # depth 0
    ("nuc", _nuc(a=9), 0.5, 10, "N", "low"),                      # depth == minDepth - 1
    ("nuc", _nuc(a=10), 0.5, 10, "A", "single"),                  # depth == minDepth
    ("nuc", _nuc(a=5, c=5), 0.5, 1, "M", "ambiguous"),            # need 5: a tie at the cut
    ("nuc", _nuc(a=6, c=4), 0.5, 1, "A", "single"),               # need 5
    ("nuc", _nuc(a=6, c=4), 0.75, 1, "M", "ambiguous"),           # need 8
    ("nuc", _nuc(a=9, c=1), 0.9, 1, "A", "single"),               # need 9
    ("nuc", _nuc(a=9, c=1), 1.0, 1, "M", "ambiguous"),            # need 10
    ("nuc", _nuc(a=9, c=1), 1e-9, 1, "A", "single"),              # need 1
    ("nuc", _nuc(a=1, t=9), 1e-9, 1, "T", "single"),
    ("nuc", _nuc(g=2**32 - 1), 1.0, 1, "G", "single"),            # the highest count a cell can hold
    ("nuc", _nuc(t=2**32 - 1), 0.5, 2**32 - 1, "T", "single"),
    ("aa", _aa(D=3), 0.5, 1, "D", "single"),
    ("aa", _aa(stop=8, Y=1), 0.75, 1, "*", "single"),             # need 7
    ("aa", _aa(gap=4), 1.0, 1, "-", "deleted"),
    ("aa", _aa(gap=4, A=4), 0.5, 1, "X", "ambiguous"),
    ("aa", _aa(K=5, R=3, stop=1), 0.9, 1, "X", "ambiguous"),      # need 9
    ("aa", _aa(K=5, R=3, stop=1), 0.5, 1, "K", "single"),         # need 5
    ("aa", [1] * len(AA_VALID), 1e-9, 1, "X", "ambiguous"),       # a 22-way tie
    ("aa", _aa(), 1.0, 1, "X", "low"),
    ("aa", _aa(W=2), 0.5, 3, "X", "low"),
    ("aa", _aa(Y=2**32 - 1), 1.0, 1, "Y", "single"),
]
