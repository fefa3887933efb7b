"""The numpy reference of the pairwise distances (K10, silo_gpu_distance_pack / silo_gpu_distance_pairs) — test infrastructure only.

Pinned against a plain double loop by tests/test_pair_distances_reference.py and used by tests/test_pair_distances_gpu.py and
tests/test_distance_matrix_gpu.py.
"""
import numpy as np

NUC_VALID = "-ACGT"
AA_VALID = "-ACDEFGHIKLMNPQRSTVWY*"
NUC_CHARS = "-ACGTRYSWKMBDHVN"
AA_CHARS = "-ACDEFGHIKLMNPQRSTVWYBZ*X"
NOT_VALID = 0xFF


def code_table(valid_chars):
    """uint8 [256]: the index of a byte among the valid mutation symbols, NOT_VALID for every other byte."""
    table = np.full(256, NOT_VALID, dtype=np.uint8)
    for index, char in enumerate(valid_chars):
        table[ord(char)] = index
    return table


def code_bits(valid_chars):
    """Planes that hold the index of a valid symbol: 3 for the 5 nucleotide symbols, 5 for the 22 amino acid symbols."""
    return (len(valid_chars) - 1).bit_length()


def pack_planes(chars, valid_chars):
    """uint64 [n][1 + code bits][ceil(P / 64)]: what silo_gpu_distance_pack leaves for chars uint8 [n][P].  Plane 0: the position
    holds a valid symbol; plane 1 + k: bit k of its index, 0 where not valid; bit b of word w = position 64 w + b; bits at or past
    P are zero."""
    chars = np.asarray(chars, dtype=np.uint8)
    n, positions = chars.shape
    words = (positions + 63) // 64
    codes = code_table(valid_chars)[chars]
    valid = codes != NOT_VALID
    planes = [valid] + [valid & ((codes >> k) & 1).astype(bool) for k in range(code_bits(valid_chars))]
    padded = np.zeros((n, len(planes), words * 64), dtype=np.uint8)
    for k, plane in enumerate(planes):
        padded[:, k, :positions] = plane
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(n, len(planes), words)


def pair_distances(chars, valid_chars, max_elements=1 << 25):
    """uint32 [n][n][2] for chars uint8 [n][P]: cell (i, j) = (positions where rows i and j both hold a valid symbol and the two
    differ, positions where both hold a valid symbol).  The whole square is filled (it is symmetric).  Rows are taken in chunks
    of at most max_elements / (n P) so that the temporaries of a chunk stay small."""
    chars = np.asarray(chars, dtype=np.uint8)
    n, positions = chars.shape
    out = np.zeros((n, n, 2), dtype=np.uint32)
    if n == 0 or positions == 0:
        return out
    valid = code_table(valid_chars)[chars] != NOT_VALID
    step = max(1, max_elements // (n * positions))
    for begin in range(0, n, step):
        end = min(n, begin + step)
        both = valid[begin:end, None, :] & valid[None, :, :]
        out[begin:end, :, 1] = both.sum(axis=-1)
        both &= chars[begin:end, None, :] != chars[None, :, :]
        out[begin:end, :, 0] = both.sum(axis=-1)
    return out
