"""The numpy reference of the pairwise sums of count tables (K24, silo_gpu_table_pair_sums) and of the rows that MeanDistances /
AminoAcidMeanDistances make of them — test infrastructure only.

Pinned against a plain loop over positions, symbols and pairs of tables, against the sums of tests/pair_distances_reference.py over
pairs of rows and against a loop over characters by tests/test_mean_distances_reference.py, and used by
tests/test_table_pair_sums_gpu.py and tests/test_mean_distances_gpu.py.

No sum here can wrap: a position's term is below 2^64 (a coverage is below 2^32) and is formed in uint64; the terms of a range are
summed as Python integers, from the exact uint64 sums of their low and their high 32 bits (fewer than 2^32 terms of 32 bits).
"""
import numpy as np

MAX_TABLES = 64        # SILO_GPU_MAX_PAIR_SUM_TABLES
MAX_RANGES = 256       # SILO_GPU_MAX_PAIR_SUM_RANGES
WORDS = 5              # SILO_GPU_PAIR_SUM_WORDS: diff_lo, diff_hi, cmp_lo, cmp_hi, sites
TILE = 16              # SILO_GPU_PAIR_SUM_TILE: tables of a side of a block's tile of pairs
POSITION_TILE = 16     # SILO_GPU_PAIR_SUM_POSITION_TILE: positions a block stages at a time
CHUNK = 128            # SILO_GPU_PAIR_SUM_CHUNK: positions of a range that a block owns
MAX_ROWS = 65536       # of a MeanDistances response before limit and offset
MASK64 = (1 << 64) - 1


def _exact_sum(terms):
    """Python integers [...]: the sums over the last axis of uint64 [...][n]."""
    low = (terms & np.uint64(0xFFFFFFFF)).sum(axis=-1, dtype=np.uint64)
    high = (terms >> np.uint64(32)).sum(axis=-1, dtype=np.uint64)
    return high.astype(object) * (1 << 32) + low.astype(object)


def pair_index(g, h, n_tables):
    """Where the record of the pair g <= h lies among the n_tables (n_tables + 1) / 2 of a range: the order g, h."""
    return g * n_tables - g * (g + 1) // 2 + h


def pair_sums(tables, ranges):
    """For tables uint32 [T][P][n_symbols] and ranges [(first, end)] (0-based, end exclusive, any order, overlaps allowed): Python
    integers [n_ranges][T (T + 1) / 2][3] = (differences, compared, sites) per range and pair g <= h in the order g, h.  With cov the
    sum of a position's counts and shared = sum_s c_g[s] c_h[s], summed over the range's positions:
        g < h    differences cov_g cov_h - shared; compared cov_g cov_h; sites: cov_g cov_h > 0 and shared == 0
        g == h   differences (cov^2 - shared) / 2; compared cov (cov - 1) / 2; sites: at least two symbols with a count above 0"""
    tables = np.asarray(tables, dtype=np.uint32)
    n_tables, positions, _ = tables.shape
    wide = tables.astype(np.uint64)
    coverage = wide.sum(axis=-1)
    assert coverage.max(initial=0) <= 0xFFFFFFFF
    present = (tables != 0).sum(axis=-1)
    out = np.zeros((len(ranges), n_tables * (n_tables + 1) // 2, 3), dtype=object)
    for g in range(n_tables):
        shared = np.einsum("ps,hps->hp", wide[g], wide[g:])  # uint64: at most cov_g cov_h
        product = coverage[g][None, :] * coverage[g:]
        differences = product - shared
        compared = product.copy()
        sites = ((product != 0) & (shared == 0)).astype(np.uint64)
        differences[0] //= np.uint64(2)
        compared[0] = np.where(coverage[g] == 0, np.uint64(0), coverage[g] * (coverage[g] - np.uint64(1)) // np.uint64(2))
        sites[0] = present[g] >= 2
        first_pair = pair_index(g, g, n_tables)
        for r, (first, end) in enumerate(ranges):
            assert 0 <= first < end <= positions
            for k, terms in enumerate((differences, compared, sites)):
                out[r, first_pair:first_pair + n_tables - g, k] = _exact_sum(terms[:, first:end])
    return out


def pack(sums):
    """uint64 [n_ranges * pairs * 5]: the words silo_gpu_table_pair_sums leaves for the sums of pair_sums."""
    flat = np.asarray(sums, dtype=object).reshape(-1, 3)
    words = [[d & MASK64, d >> 64, c & MASK64, c >> 64, s] for d, c, s in flat.tolist()]
    return np.array(words, dtype=np.uint64).reshape(-1)


def _ratio(dividend, divisor):
    """One IEEE division of the correctly rounded doubles of two integers (Python's float of an int rounds to nearest even)."""
    return float(dividend) / float(divisor) if divisor else None


def rows(tables, group_rows, group_names, regions, sequence_name, between=True):
    """The rows of a response in the order region, g, h: tables uint32 [G][P][n_symbols] of the groups `group_names` (None: the one
    group of a request without groups) with `group_rows` rows each; regions [(name, positionFrom, positionTo)], 1-based and inclusive
    (name None: the one region of a request without regions)."""
    n_groups = len(group_names)
    group_rows = [int(count) for count in group_rows]
    sums = pair_sums(tables, [(first - 1, last) for _, first, last in regions])
    out = []
    for (region, first, last), of_region in zip(regions, sums):
        for g in range(n_groups):
            for h in range(g, n_groups if between else g + 1):
                differences, compared, sites = (int(v) for v in of_region[pair_index(g, h, n_groups)])
                pairs = group_rows[g] * (group_rows[g] - 1) // 2 if g == h else group_rows[g] * group_rows[h]
                out.append({
                    "region": region, "positionFrom": first, "positionTo": last, "sequenceName": sequence_name, "group": group_names[g],
                    "otherGroup": group_names[h], "count": int(group_rows[g]), "otherCount": int(group_rows[h]), "pairs": str(pairs),
                    "differences": str(differences), "comparedPositions": str(compared), "segregatingSites": sites if g == h else None,
                    "fixedDifferences": sites if g != h else None, "meanDistance": _ratio(differences, pairs),
                    "meanCompared": _ratio(compared, pairs), "distancePerSite": _ratio(differences, compared),
                })
    return out
