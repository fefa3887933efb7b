"""The numpy reference of the bit-per-pair matrix and of its connected components (K12, silo_gpu_distance_within /
silo_gpu_adjacency_components) — test infrastructure only.

Pinned against tests/pair_distances_reference.py, a plain character double loop and a breadth-first search by
tests/test_clusters_reference.py and used by tests/test_distance_within_gpu.py, tests/test_adjacency_components_gpu.py and
tests/test_clusters_gpu.py.
"""
import numpy as np

from tests.pair_distances_reference import pack_planes

NO_BOUND = 0xFFFFFFFF  # max_distance: no bound on the distance


def adjacency_words(n):
    """SILO_GPU_ADJACENCY_WORDS: 64-bit words per row of the bit matrix."""
    return (n + 63) // 64


def pack_bits(linked):
    """bool [n][n] -> uint64 [n][ceil(n / 64)]: bit (j & 63) of word (i, j >> 6) = linked[i, j]; bits at or past n are zero."""
    n = len(linked)
    padded = np.zeros((n, adjacency_words(n) * 64), dtype=np.uint8)
    padded[:, :n] = linked
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(n, adjacency_words(n))


def unpack_bits(adjacency, n):
    """uint64 [n][ceil(n / 64)] -> bool [n][n]; bits at or past n are dropped."""
    words = np.ascontiguousarray(np.asarray(adjacency, dtype="<u8").reshape(n, adjacency_words(n)))
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")[:, :n].astype(bool)


def pair_counts(chars, valid_chars, max_elements=1 << 22):
    """(differing, compared), uint32 [n][n] each, from the words of pack_planes with np.bitwise_count: what silo_gpu_distance_pairs
    counts, for the whole square.  Rows are taken in chunks of at most max_elements / (n words) rows."""
    chars = np.asarray(chars, dtype=np.uint8)
    n, positions = chars.shape
    differing = np.zeros((n, n), dtype=np.uint32)
    compared = np.zeros((n, n), dtype=np.uint32)
    if n == 0 or positions == 0:
        return differing, compared
    planes = pack_planes(chars, valid_chars)
    words = planes.shape[2]
    step = max(1, max_elements // (n * words))
    for begin in range(0, n, step):
        mine = planes[begin:begin + step]
        both = mine[:, None, 0, :] & planes[None, :, 0, :]
        unequal = np.zeros_like(both)
        for k in range(1, planes.shape[1]):
            unequal |= mine[:, None, k, :] ^ planes[None, :, k, :]
        compared[begin:begin + step] = np.bitwise_count(both).sum(axis=-1, dtype=np.uint32)
        differing[begin:begin + step] = np.bitwise_count(both & unequal).sum(axis=-1, dtype=np.uint32)
    return differing, compared


def linked_pairs(differing, compared, max_distance, min_compared):
    """bool [n][n]: i != j and differing <= max_distance and compared >= min_compared (NO_BOUND / 0: no bound)."""
    linked = (differing.astype(np.uint64) <= max_distance) & (compared.astype(np.uint64) >= min_compared)
    np.fill_diagonal(linked, False)
    return linked


def within_adjacency(chars, valid_chars, max_distance, min_compared):
    """uint64 [n][ceil(n / 64)] for chars uint8 [n][P]: what silo_gpu_distance_within leaves."""
    return pack_bits(linked_pairs(*pair_counts(chars, valid_chars), max_distance, min_compared))


def components(adjacency, n=None):
    """uint32 [n]: per row the lowest row of its connected component, for a symmetric bit matrix uint64 [n][ceil(n / 64)] (or a
    bool matrix [n][n]).  A union-find whose roots are the lowest rows: row by row, the roots of the row and of its neighbours are
    found (the finds of one row in one numpy step) and linked under the lowest of them."""
    adjacency = np.asarray(adjacency)
    linked = adjacency if adjacency.dtype == bool else unpack_bits(adjacency, len(adjacency) if n is None else n)
    n = len(linked)
    parent = np.arange(n, dtype=np.int64)
    for i in range(n):
        members = np.flatnonzero(linked[i])
        if len(members) == 0:
            continue
        members = np.append(members, i)
        roots = parent[members]
        while True:
            above = parent[roots]
            if np.array_equal(above, roots):
                break
            roots = above
        parent[roots] = roots.min()
        parent[members] = roots.min()
    while True:
        above = parent[parent]
        if np.array_equal(above, parent):
            return parent.astype(np.uint32)
        parent = above


def cluster_sizes(labels):
    """uint32 [n]: per row the number of rows that share its label."""
    labels = np.asarray(labels)
    return np.bincount(labels, minlength=len(labels))[labels].astype(np.uint32)


def has_chain(linked, labels):
    """Whether some two rows of one component are not linked themselves: what tells single linkage from a complete one."""
    labels = np.asarray(labels)
    same = labels[:, None] == labels[None, :]
    np.fill_diagonal(same, False)
    return bool((same & ~linked).any())
