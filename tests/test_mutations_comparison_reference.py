"""tests/mutations_comparison_reference.py (the numpy reference of K17 and of the rows of MutationsComparison) against a plain loop
over positions, symbols and groups that applies the rule on its own, against rows worked out by hand, and the constants of K17 that
silo_amd/binding.py restates against include/silo_gpu.h; runs without a GPU."""
import math
import os
import re

import numpy as np
import pytest

from tests.consensus_reference import VALID
from tests.mutations_comparison_reference import (FIRST_CAPACITY, HAND_MADE, HEADER_WORDS, MAX_TABLES, THREADS, compare_tables, comparison_rows,
                                                  group_tables, unpack)

SETTINGS = [(0.05, 0.0), (0.05, 0.5), (0.5, 0.0), (1.0, 0.0), (0.0, 0.0), (0.05, 0.25), (0.0, 1.0), (0.3, 0.1)]


def _loop(tables, reference_index, min_proportion, min_difference):
    """[(position, symbol, [(count, coverage) per table], difference, [passes per table])] in ascending order, by the rule as the
    issue words it, in Python integers and floats."""
    n_tables, positions, n_symbols = len(tables), len(tables[0]), len(tables[0][0])
    selected = []
    for p in range(positions):
        coverage = [sum(tables[t][p]) for t in range(n_tables)]
        for s in range(n_symbols):
            passes, proportions = [], []
            for t in range(n_tables):
                count = tables[t][p][s]
                if coverage[t] == 0:
                    passes.append(False)
                    continue
                bound = 0 if min_proportion == 0 else int(math.ceil(float(coverage[t]) * min_proportion) - 1)
                passes.append(count > bound)
                proportions.append(count / coverage[t])
            difference = max(proportions) - min(proportions) if len(proportions) >= 2 else 0.0
            if s != reference_index[p] and any(passes) and difference >= min_difference:
                selected.append((p, s, [(tables[t][p][s], coverage[t]) for t in range(n_tables)], difference, passes))
    return selected


def _skewed(rng, alphabet, tables, positions):
    """Count tables with one heavy symbol at most positions — the same in most tables, another in some —, light ones beside it,
    shallow and empty positions, and tables that are empty at a position."""
    n_symbols = len(VALID[alphabet])
    counts = rng.integers(0, 4, size=(tables, positions, n_symbols)).astype(np.uint32)
    counts[rng.random(counts.shape) < 0.6] = 0
    shared = rng.integers(0, n_symbols, size=(1, positions))
    heavy = np.where(rng.random((tables, positions)) < 0.8, shared, rng.integers(0, n_symbols, size=(tables, positions)))
    weight = rng.choice(np.array([0, 3, 40, 1000], dtype=np.uint32), size=(tables, positions), p=[0.1, 0.3, 0.3, 0.3])
    np.put_along_axis(counts, heavy[..., None], np.take_along_axis(counts, heavy[..., None], axis=-1) + weight[..., None], axis=-1)
    counts[rng.random((tables, positions)) < 0.1] = 0
    counts[:, rng.random(positions) < 0.05] = 0
    return counts


def _reference_index(rng, alphabet, positions):
    index = rng.integers(0, len(VALID[alphabet]), size=positions).astype(np.uint8)
    index[rng.random(positions) < 0.1] = 0xFF
    return index


def _same(got, want):
    records, cells, difference, passes = got
    assert records.dtype == np.uint32 and cells.dtype == np.uint32 and difference.dtype == np.float64
    assert records.tolist() == [[p, s] for p, s, _, _, _ in want]
    assert cells.tolist() == [[list(cell) for cell in of_tables] for _, _, of_tables, _, _ in want]
    assert difference.tolist() == [spread for _, _, _, spread, _ in want]  # exact: the same IEEE divisions and subtraction
    assert passes.tolist() == [flags for _, _, _, _, flags in want]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("tables,positions", [(2, 40), (3, 70), (9, 30)])
def test_random_tables_match_a_plain_loop(alphabet, tables, positions):
    rng = np.random.default_rng(1700 + tables + positions)
    counts = _skewed(rng, alphabet, tables, positions)
    reference_index = _reference_index(rng, alphabet, positions)
    sizes = set()
    for min_proportion, min_difference in SETTINGS:
        want = _loop(counts.tolist(), reference_index.tolist(), min_proportion, min_difference)
        _same(compare_tables(counts, reference_index, min_proportion, min_difference), want)
        sizes.add(len(want))
    assert len(sizes) >= 4 and min(sizes) < max(sizes) // 2  # the settings decide something


@pytest.mark.parametrize("row", range(len(HAND_MADE)))
def test_hand_made_rows(row):
    what, counts, reference_index, min_proportion, min_difference, expected = HAND_MADE[row]
    tables = np.array(counts, dtype=np.uint32)[:, None, :]
    got = compare_tables(tables, np.array([reference_index], dtype=np.uint8), min_proportion, min_difference)
    _same(got, _loop(tables.tolist(), [reference_index], min_proportion, min_difference))
    assert got[0].tolist() == [[0, symbol] for symbol in sorted(expected)], what
    assert got[2].tolist() == [expected[symbol] for symbol in sorted(expected)], what
    for (_, symbol), of_tables in zip(got[0].tolist(), got[1].tolist()):
        assert of_tables == [[table[symbol], sum(table)] for table in counts], what


def test_the_hand_made_rows_cover_what_the_rule_distinguishes():
    assert {min_proportion for _, _, _, min_proportion, _, _ in HAND_MADE} >= {0.0, 0.05, 1.0}
    assert any(reference_index == 0xFF for _, _, reference_index, _, _, _ in HAND_MADE)
    assert any(max(max(table) for table in counts) == 2**32 - 1 for _, counts, _, _, _, _ in HAND_MADE)
    assert any(counts[0] == counts[1] and expected and set(expected.values()) == {0.0} for _, counts, _, _, _, expected in HAND_MADE)
    assert any(not any(any(table) for table in counts) for _, counts, _, _, _, _ in HAND_MADE)  # no table covered
    assert any(sum(any(table) for table in counts) == 1 and expected for _, counts, _, _, _, expected in HAND_MADE)  # one table covered
    assert any(min_difference in expected.values() and min_difference > 0 for _, _, _, _, min_difference, expected in HAND_MADE)


def test_rows_in_the_order_position_symbol_group():
    reference = "ACGTN"
    chars = [np.frombuffer(b"ACGTA" b"CCGTA" b"-CGNA" b"ACTTA", dtype=np.uint8).reshape(4, 5), np.frombuffer(b"CCGTT" b"CCGTT", dtype=np.uint8).reshape(2, 5),
             np.zeros((0, 5), dtype=np.uint8)]
    tables = group_tables(chars, "nuc", 5)
    assert tables.shape == (3, 5, 5) and tables[0, 0].tolist() == [1, 2, 1, 0, 0] and not tables[2].any()
    rows = comparison_rows(tables, reference, "nuc", "main", ["a", "b", "none"], 0.05, 0.0)
    assert [(row["mutation"], row["group"]) for row in rows] == [(m, g) for m in ("A1-", "A1C", "G3T", "N5A", "N5T") for g in ("a", "b", "none")]
    first = rows[3]  # A1C in a
    assert first == {"mutation": "A1C", "sequenceName": "main", "position": 1, "group": "a", "count": 1, "coverage": 4, "proportion": 0.25, "difference": 0.75}
    assert rows[4]["proportion"] == 1.0 and rows[4]["difference"] == 0.75
    assert all(row["proportion"] is None and row["count"] == 0 and row["coverage"] == 0 for row in rows if row["group"] == "none")
    assert [row["mutation"] for row in comparison_rows(tables, reference, "nuc", "main", ["a", "b", "none"], 0.05, 0.5)][::3] == ["A1C", "N5A", "N5T"]
    assert comparison_rows(np.zeros((2, 5, 5), np.uint32), reference, "nuc", "main", ["a", "b"], 0.0, 0.0) == []


def test_unpack_puts_the_records_in_order_with_their_cells():
    capacity, tables = 3, 2
    out = np.full(HEADER_WORDS + capacity * 2 + capacity * tables * 2 + 4, 0xA5A5A5A5, dtype=np.uint32)
    out[:HEADER_WORDS] = [5, 0, 0, 0]
    out[4:10] = [7, 1, 2, 4, 2, 0]
    out[10:22] = [71, 72, 73, 74, 241, 242, 243, 244, 201, 202, 203, 204]
    selected, records, cells = unpack(out, tables, capacity)
    assert selected == 5 and records.tolist() == [[2, 0], [2, 4], [7, 1]]
    assert cells.tolist() == [[[201, 202], [203, 204]], [[241, 242], [243, 244]], [[71, 72], [73, 74]]]
    out[0] = 2
    assert unpack(out, tables, capacity)[1].tolist() == [[2, 4], [7, 1]]


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_COMPARISON_TABLES == defined("SILO_GPU_MAX_COMPARISON_TABLES") == MAX_TABLES == 64
    assert binding.COMPARE_THREADS == defined("SILO_GPU_COMPARE_THREADS") == THREADS == 256
    assert binding.COMPARE_HEADER_WORDS == HEADER_WORDS == 4 and FIRST_CAPACITY == 1024
    assert "silo_gpu_mutations_compare" in binding.EXPORTED_SYMBOLS and re.search(r"\bint silo_gpu_mutations_compare\(", header)
