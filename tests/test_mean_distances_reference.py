"""tests/mean_distances_reference.py (the numpy reference of K24 and of the rows of MeanDistances) against a plain loop over
positions, symbols and pairs of tables, against the definition the tables replace — the sums of DistanceMatrix's reference
(tests/pair_distances_reference.py) over every pair of rows of two row sets —, against a loop over characters for the two kinds of
sites, the constants of K24 that silo_amd/binding.py restates against include/silo_gpu.h, and the guard that the example data set's
groups which tests/test_mean_distances_gpu.py uses decide something; runs without a GPU."""
import os
import re

import numpy as np
import pytest

from tests import dataset
from tests.consensus_reference import VALID, count_table
from tests.mean_distances_reference import CHUNK, MASK64, MAX_RANGES, MAX_ROWS, MAX_TABLES, POSITION_TILE, TILE, WORDS, pack, pair_index, pair_sums, rows
from tests.pair_distances_reference import AA_CHARS, NUC_CHARS, pair_distances

CHARS = {"nuc": NUC_CHARS, "aa": AA_CHARS}  # valid symbols, ambiguity codes and the missing symbol
# the genes of the example data set's genome (NC_045512.2), 1-based and inclusive: the regions of the tests through JSON
GENES = [("ORF1a", 266, 13468), ("ORF1b", 13468, 21555), ("S", 21563, 25384), ("ORF3a", 25393, 26220), ("E", 26245, 26472), ("M", 26523, 27191),
         ("ORF6", 27202, 27387), ("ORF7a", 27394, 27759), ("ORF7b", 27756, 27887), ("ORF8", 27894, 28259), ("N", 28274, 29533), ("ORF9b", 28284, 28577)]


def _loop(tables, ranges):
    """[[(differences, compared, sites) per pair g <= h] per range] by the statement as the issue words it, in Python integers."""
    n_tables = len(tables)
    out = []
    for first, end in ranges:
        of_range = []
        for g in range(n_tables):
            for h in range(g, n_tables):
                differences = compared = sites = 0
                for p in range(first, end):
                    of_g, of_h = [int(c) for c in tables[g][p]], [int(c) for c in tables[h][p]]
                    coverage_g, coverage_h = sum(of_g), sum(of_h)
                    shared = sum(a * b for a, b in zip(of_g, of_h))
                    if g == h:
                        assert (coverage_g * coverage_g - shared) % 2 == 0
                        differences += (coverage_g * coverage_g - shared) // 2
                        compared += coverage_g * (coverage_g - 1) // 2
                        sites += sum(1 for c in of_g if c != 0) >= 2
                    else:
                        differences += coverage_g * coverage_h - shared
                        compared += coverage_g * coverage_h
                        sites += coverage_g * coverage_h > 0 and shared == 0
                of_range.append((differences, compared, sites))
        out.append(of_range)
    return out


def _tables(rng, alphabet, n_tables, positions, high=50):
    counts = rng.integers(0, high, size=(n_tables, positions, len(VALID[alphabet]))).astype(np.uint32)
    counts[rng.random(counts.shape) < 0.5] = 0
    counts[rng.random((n_tables, positions)) < 0.15] = 0  # a table that is empty at a position
    return counts


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("n_tables,positions", [(1, 9), (2, 40), (5, 33)])
def test_random_tables_match_a_plain_loop(alphabet, n_tables, positions):
    rng = np.random.default_rng(3100 + n_tables + (alphabet == "aa"))
    ranges = [(0, positions), (0, 1), (positions - 1, positions), (positions // 3, positions // 3 + 4), (positions // 3 + 2, positions)]
    for tables in (_tables(rng, alphabet, n_tables, positions), _tables(rng, alphabet, n_tables, positions, high=2**32 // len(VALID[alphabet]))):
        got = pair_sums(tables, ranges)
        assert got.shape == (len(ranges), n_tables * (n_tables + 1) // 2, 3)
        assert [[tuple(int(v) for v in pair) for pair in of_range] for of_range in got] == _loop(tables.tolist(), ranges)
    assert positions < 30 or max(int(v) for v in got[0, :, 0]) > MASK64  # the second tables' sums need the high word


def test_pack_splits_the_sums_into_words():
    sums = np.array([[[(5 << 64) + 7, (1 << 127) + 1, 3], [0, MASK64, 0]]], dtype=object)
    assert pack(sums).tolist() == [7, 5, 1, 1 << 63, 3, 0, 0, MASK64, 0, 0]
    assert pack(sums).dtype == np.uint64
    assert [pair_index(g, h, 3) for g in range(3) for h in range(g, 3)] == list(range(6))


def _random_chars(rng, alphabet, n, positions):
    chars = np.frombuffer(CHARS[alphabet].encode(), dtype=np.uint8)
    weights = np.where(np.isin(chars, np.frombuffer(VALID[alphabet].encode(), dtype=np.uint8)), 6.0, 1.0)  # N, ambiguity codes and '-' among them
    matrix = rng.choice(chars, size=(n, positions), p=weights / weights.sum())
    common = rng.choice(chars[1:5], size=positions)  # most rows agree at most positions, as sequences do
    return np.where(rng.random((n, positions)) < 0.6, common[None, :], matrix).astype(np.uint8)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_the_sums_of_pair_distances_over_two_row_sets(alphabet):
    """The statement against the definition it replaces, on 40 rows x 60 positions: disjoint, overlapping and identical row sets."""
    rng = np.random.default_rng(3200 + (alphabet == "aa"))
    chars = _random_chars(rng, alphabet, 40, 60)
    assert not np.isin(chars, np.frombuffer(VALID[alphabet].encode(), dtype=np.uint8)).all()
    distances = pair_distances(chars, VALID[alphabet]).astype(np.int64)  # [40][40][2] = (distance, compared)
    sets = [np.arange(0, 15), np.arange(15, 40), np.arange(10, 30), np.arange(0, 15), np.array([7])]
    tables = np.stack([count_table(chars[rows_of], alphabet) for rows_of in sets])
    got = pair_sums(tables, [(0, 60)])[0]
    for g, rows_g in enumerate(sets):
        for h in range(g, len(sets)):
            rows_h = sets[h]
            if g == h:  # the unordered pairs i < j of the set
                square = distances[np.ix_(rows_g, rows_g)]
                want = [int(np.triu(square[..., k], 1).sum()) for k in range(2)]
            else:  # the rectangle: a row of both sets pairs with itself, distance 0, compared where it is valid
                want = [int(distances[np.ix_(rows_g, rows_h)][..., k].sum()) for k in range(2)]
            assert [int(v) for v in got[pair_index(g, h, len(sets))][:2]] == want, (g, h)
    # a region: the distances of the region's columns alone
    part = pair_distances(chars[:, 20:45], VALID[alphabet]).astype(np.int64)
    got = pair_sums(tables, [(20, 45)])[0]
    assert [int(v) for v in got[pair_index(0, 1, len(sets))][:2]] == [int(part[np.ix_(sets[0], sets[1])][..., k].sum()) for k in range(2)]
    assert int(got[pair_index(0, 1, len(sets))][0]) > 0


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_sites_against_a_loop_over_characters(alphabet):
    rng = np.random.default_rng(3300 + (alphabet == "aa"))
    chars = _random_chars(rng, alphabet, 30, 80)
    chars[:12, 5] = ord("A")  # a fixed difference: no symbol in both sets
    chars[12:, 5] = ord("C")
    chars[12:, 6] = ord("N" if alphabet == "nuc" else "X")  # the other set is not covered: no fixed difference
    chars[:, 7] = ord("G")  # one symbol: not segregating
    sets = [list(range(0, 12)), list(range(12, 30))]
    valid = set(VALID[alphabet].encode())
    symbols = [[{int(chars[r, p]) for r in rows_of} & valid for p in range(80)] for rows_of in sets]
    tables = np.stack([count_table(chars[rows_of], alphabet) for rows_of in sets])
    for first, end in ((0, 80), (5, 8), (40, 80)):
        got = pair_sums(tables, [(first, end)])[0]
        segregating = [sum(len(symbols[g][p]) >= 2 for p in range(first, end)) for g in range(2)]
        fixed = sum(bool(symbols[0][p]) and bool(symbols[1][p]) and not symbols[0][p] & symbols[1][p] for p in range(first, end))
        assert [int(got[pair_index(0, 0, 2)][2]), int(got[pair_index(1, 1, 2)][2]), int(got[pair_index(0, 1, 2)][2])] == segregating + [fixed]
    assert fixed == 0 and int(pair_sums(tables, [(5, 8)])[0][pair_index(0, 1, 2)][2]) == 1


def test_rows_in_the_order_region_group_other_group():
    tables = np.zeros((2, 4, 5), dtype=np.uint32)
    tables[0, :, 1] = [3, 3, 0, 2]  # A
    tables[0, :, 2] = [0, 0, 0, 1]  # C
    tables[1, :, 1] = [2, 0, 2, 1]
    tables[1, :, 3] = [0, 2, 0, 1]  # G
    got = rows(tables, [3, 2], ["a", "b"], [("all", 1, 4), ("last", 4, 4)], "main")
    assert [(row["region"], row["group"], row["otherGroup"]) for row in got] == [(r, g, h) for r in ("all", "last") for g, h in (("a", "a"), ("a", "b"), ("b", "b"))]
    assert got[0] == {"region": "all", "positionFrom": 1, "positionTo": 4, "sequenceName": "main", "group": "a", "otherGroup": "a", "count": 3, "otherCount": 3,
                      "pairs": "3", "differences": "2", "comparedPositions": "9", "segregatingSites": 1, "fixedDifferences": None, "meanDistance": 2 / 3,
                      "meanCompared": 3.0, "distancePerSite": 2 / 9}
    assert got[1] == {"region": "all", "positionFrom": 1, "positionTo": 4, "sequenceName": "main", "group": "a", "otherGroup": "b", "count": 3, "otherCount": 2,
                      "pairs": "6", "differences": "10", "comparedPositions": "18", "segregatingSites": None, "fixedDifferences": 1, "meanDistance": 10 / 6,
                      "meanCompared": 3.0, "distancePerSite": 10 / 18}
    only_within = rows(tables, [3, 2], ["a", "b"], [("all", 1, 4)], "main", between=False)
    assert only_within == [got[0], got[2]]
    empty = rows(np.zeros((1, 4, 5), dtype=np.uint32), [0], [None], [(None, 1, 4)], "main")
    assert empty == [{"region": None, "positionFrom": 1, "positionTo": 4, "sequenceName": "main", "group": None, "otherGroup": None, "count": 0, "otherCount": 0,
                      "pairs": "0", "differences": "0", "comparedPositions": "0", "segregatingSites": 0, "fixedDifferences": None, "meanDistance": None,
                      "meanCompared": None, "distancePerSite": None}]


def test_the_doubles_are_the_correctly_rounded_integers_divided_once():
    tables = np.zeros((2, 3, 5), dtype=np.uint32)
    tables[0, :, 1] = 2**32 - 1
    tables[1, :, 2] = 2**32 - 3
    (row,) = [row for row in rows(tables, [2**32 - 1, 2**32 - 3], ["a", "b"], [(None, 1, 3)], "main") if row["group"] != row["otherGroup"]]
    differences, pairs = 3 * (2**32 - 1) * (2**32 - 3), (2**32 - 1) * (2**32 - 3)
    assert row["differences"] == row["comparedPositions"] == str(differences) and row["pairs"] == str(pairs) and differences > 2**65
    assert row["meanDistance"] == float(differences) / float(pairs) and row["distancePerSite"] == 1.0 and row["fixedDifferences"] == 3


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_PAIR_SUM_TABLES == defined("SILO_GPU_MAX_PAIR_SUM_TABLES") == MAX_TABLES == 64
    assert binding.MAX_PAIR_SUM_RANGES == defined("SILO_GPU_MAX_PAIR_SUM_RANGES") == MAX_RANGES == 256
    assert binding.PAIR_SUM_WORDS == defined("SILO_GPU_PAIR_SUM_WORDS") == WORDS == 5
    assert binding.PAIR_SUM_TILE == defined("SILO_GPU_PAIR_SUM_TILE") == TILE == 16
    assert binding.PAIR_SUM_POSITION_TILE == defined("SILO_GPU_PAIR_SUM_POSITION_TILE") == POSITION_TILE == 16
    assert binding.PAIR_SUM_CHUNK == defined("SILO_GPU_PAIR_SUM_CHUNK") == CHUNK == 128 and CHUNK % POSITION_TILE == 0
    assert MAX_ROWS == 65536 < MAX_RANGES * (MAX_TABLES * (MAX_TABLES + 1) // 2)  # the row cap can be reached
    assert "silo_gpu_table_pair_sums" in binding.EXPORTED_SYMBOLS and re.search(r"\bint silo_gpu_table_pair_sums\(", header)


def example_groups(store):
    """(chars uint8 [100][P] of the example data set's rows in `store`, bool [100]: the row's lineage is B.1.1.7 or a sublineage).  From
    the data set's own files: the aligned sequences, a row without one as the missing symbol throughout, and the lineages with their
    aliases resolved."""
    data = dataset.load_example_dataset()
    is_aa = store != "main"
    sequences = data["aa" if is_aa else "nuc"][store]
    positions = len((data["aa_references"] if is_aa else data["nuc_references"])[store])
    missing = "X" if is_aa else "N"
    chars = np.array([list((sequence if sequence is not None else missing * positions).encode()) for sequence in sequences], dtype=np.uint8)
    assert chars.shape == (len(data["keys"]), positions)

    def resolved(lineage):
        head, _, tail = (lineage or "").partition(".")
        full = data["alias"].get(head)
        full = full if isinstance(full, str) and full else head
        return full + ("." + tail if tail else "")

    lineage = np.array([resolved(name) == "B.1.1.7" or resolved(name).startswith("B.1.1.7.") for name in data["lineages"]])
    return chars, lineage


def test_the_example_groups_decide_something():
    """The non-vacuity guard of tests/test_mean_distances_gpu.py, of the reference first: B.1.1.7 with its sublineages (51 rows)
    against the other 49, over the genome and its genes and over the gene S in amino acids."""
    chars, lineage = example_groups("main")
    assert (int(lineage.sum()), int((~lineage).sum())) == (51, 49)
    tables = np.stack([count_table(chars[lineage], "nuc"), count_table(chars[~lineage], "nuc")])
    regions = [(None, 1, chars.shape[1])] + GENES
    got = rows(tables, [51, 49], ["lineage", "others"], regions, "main")
    between = [row for row in got if row["group"] != row["otherGroup"]]
    within = [row for row in got if row["group"] == row["otherGroup"]]
    assert all(int(row["differences"]) > 0 for row in got if row["region"] in (None, "S", "ORF1a", "N"))
    assert between[0]["region"] is None and between[0]["fixedDifferences"] > 0
    assert sum(row["fixedDifferences"] > 0 for row in between if row["region"] is not None) >= 2  # some genes carry them, E does not
    assert [row["fixedDifferences"] for row in between if row["region"] == "E"] == [0]
    for row in within:
        if row["region"] in (None, "S", "ORF1a", "N"):
            assert 0 < row["segregatingSites"] < row["positionTo"] - row["positionFrom"] + 1, row
    chars, lineage = example_groups("S")
    tables = np.stack([count_table(chars[lineage], "aa"), count_table(chars[~lineage], "aa")])
    a, ab, b = rows(tables, [51, 49], ["lineage", "others"], [(None, 1, chars.shape[1])], "S")
    # (no amino acid of S is fixed between the two groups in this data set: the genome's regions above carry the fixed differences)
    assert int(ab["differences"]) > 0 and ab["fixedDifferences"] == 0 and 0 < a["segregatingSites"] < chars.shape[1] and 0 < b["segregatingSites"] < chars.shape[1]
