"""The numpy statement of K23 (tests/region_counts_reference.py) against a plain loop over characters and against the whole-sequence
statement of K22, the host colouring of regions into chunks, the constants of the binding against the header, and — on the CPU — the
guard that keeps the GPU tests from being vacuous: every threshold they ask for selects a row and leaves a row out on its fixture and
region, and every action they send has a region whose count lies strictly between 0 and the total."""
import os
import re

import numpy as np
import pytest

from tests import cell_counts_reference as whole
from tests import region_counts_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _values_by_loop(rows, reference, alphabet, ranges, kinds_mask):
    """value(r, g) character by character, by the rule of tests/cell_counts_reference.py's docstring."""
    out = np.zeros((len(ranges), len(rows)), dtype=np.uint32)
    missing = "N" if alphabet == "nuc" else "X"
    for g, (first, end) in enumerate(ranges):
        for r, row in enumerate(rows):
            for p in range(first, end):
                c = row[p]
                kind = 2 if c == missing else 3 if c not in whole.VALID[alphabet] else None if c == reference[p] else 1 if c == "-" else 0
                out[g, r] += kind is not None and (kinds_mask >> kind) & 1
    return out


def _sym(rows, alphabet):
    return np.array([[whole.CHARS[alphabet].index(c) for c in row] for row in rows], dtype=np.uint8)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_numpy_matches_a_character_loop(alphabet):
    rng = np.random.default_rng(6)
    chars = whole.CHARS[alphabet]
    rows = ["".join(rng.choice(list(chars), size=40)) for _ in range(60)]
    rows.append(chars[-1] * 40)
    ranges = [(0, 40), (0, 1), (39, 40), (3, 9), (9, 10), (12, 33)]
    for reference in ("".join(rng.choice(list(whole.VALID[alphabet][1:]), size=40)), "".join(rng.choice(list(chars), size=40))):  # the second: symbols that are not valid
        for mask in range(1, 16):
            got = ref.values(_sym(rows, alphabet), _sym([reference], alphabet)[0], alphabet, ranges, mask)
            assert got.dtype == np.uint32 and np.array_equal(got, _values_by_loop(rows, reference, alphabet, ranges, mask)), mask
        assert ref.values(_sym(rows, alphabet), _sym([reference], alphabet)[0], alphabet, ranges, 4)[:, -1].tolist() == [40, 1, 1, 6, 1, 21]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_the_whole_sequence_region_is_the_whole_sequence_value(alphabet):
    from tests.test_grouped_kernels_gpu import POSITIONS, _matrix

    sym = _matrix(alphabet)[:3000]
    table = whole.cells(sym, sym[0], alphabet)
    for mask in range(1, 16):
        assert np.array_equal(ref.values(sym, sym[0], alphabet, [(0, POSITIONS)], mask)[0], whole.values(table, mask))
    parts = ref.values(sym, sym[0], alphabet, [(0, 5), (5, 6), (6, POSITIONS)], 15)
    assert np.array_equal(parts.sum(axis=0), whole.values(table, 15)) and parts.max(axis=1).min() > 0


def test_selection_counts_and_words():
    column = np.array([0, 3, 0xFFFFFFFF, 7, 3], dtype=np.uint32)
    assert ref.selected(column, 4, 1, 7).tolist() == [False, True, False, True, False]
    assert ref.selected(column, 5).tolist() == [True] * 5 and not ref.selected(column, 5, 4, 3).any()
    assert ref.counts(np.stack([column, column]), [1, 1, 1, 0, 1], [(3, 3), (0, 0xFFFFFFFF)]).tolist() == [2, 4]
    assert ref.bitset_words([1, 0, 1] + [0] * 61 + [1], 2).tolist() == [5, 1]
    assert ref.response_rows(["a"], [(4, 9)], [2], 7) == [{"region": "a", "positionFrom": 5, "positionTo": 9, "count": 2, "total": 7}]


def _check_colouring(ranges, max_regions):
    chunks = ref.colour(ranges, max_regions)
    assert sorted(g for chunk in chunks for g in chunk) == list(range(len(ranges)))  # every region exactly once
    for chunk in chunks:
        assert 1 <= len(chunk) <= max_regions
        for before, after in zip(chunk, chunk[1:]):  # ascending and disjoint: what silo_gpu_region_cell_values takes
            assert ranges[before][1] <= ranges[after][0]
    return chunks


def test_the_colouring():
    from tests.test_region_cell_count_gpu import action_regions, many_regions

    assert _check_colouring([(0, 5), (5, 9), (9, 10)], 256) == [[0, 1, 2]]
    assert _check_colouring([(9, 10), (0, 5), (5, 9)], 256) == [[1, 2, 0]]
    assert _check_colouring([(0, 5), (4, 9), (8, 10), (0, 10)], 256) == [[0, 2], [3], [1]]  # by start, ties in request order: 0, 3, 1, 2
    assert _check_colouring([(0, 5), (5, 9), (9, 10)], 2) == [[0, 1], [2]]
    assert _check_colouring([(3, 4)] * 5, 256) == [[0], [1], [2], [3], [4]]
    assert [len(chunk) for chunk in _check_colouring([(p, p + 1) for p in range(300)], 256)] == [256, 44]
    rng = np.random.default_rng(8)
    for _ in range(50):
        starts = rng.integers(0, 1000, size=int(rng.integers(1, 257)))
        _check_colouring([(int(a), int(a + rng.integers(1, 200))) for a in starts], int(rng.integers(1, 257)))
    assert len(_check_colouring([(first - 1, last) for _, first, last, _, _ in many_regions()], 256)) == 2
    assert len(_check_colouring([(first - 1, last) for _, first, last, _, _ in action_regions()], 256)) > 2
    # the budget: a chunk's columns for the largest partition stay within it, but a chunk always holds a region
    assert ref.chunk_regions(32) == 256 and ref.chunk_regions(156_256) == 6 and ref.chunk_regions(1 << 22) == 1
    for row_words in (32, 4096, 156_256):
        assert ref.chunk_regions(row_words) * row_words * 256 <= ref.REGION_VALUE_BUDGET_BYTES


def test_the_constants_of_the_binding_are_the_headers():
    from silo_amd import binding

    header = open(os.path.join(ROOT, "include", "silo_gpu.h")).read()
    assert int(re.search(r"#define SILO_GPU_MAX_REGIONS (\d+)", header).group(1)) == binding.MAX_REGIONS == ref.MAX_REGIONS
    assert "#define SILO_GPU_REGION_VALUE_SCRATCH_BYTES(positions) ((size_t)(positions) * 7u + 8192u)" in header
    assert binding.region_value_scratch_bytes(29903) == 29903 * 7 + 8192
    for entry in ("silo_gpu_region_cell_values", "silo_gpu_bitset_from_values", "silo_gpu_count_values"):
        assert entry in binding.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % entry, header)
    engine_header = open(os.path.join(ROOT, "lapis-silo_amd", "host", "query_engine.h")).read()
    assert "REGION_VALUE_BUDGET_BYTES = size_t{256} << 20" in engine_header and ref.REGION_VALUE_BUDGET_BYTES == 256 << 20


# ---- the guard: no threshold of the GPU tests is vacuous on its fixture and region ---------------------------------------------
def _cuts(mask):
    return 0 < int(np.asarray(mask).sum()) < len(mask)


def test_every_json_threshold_cuts_its_fixture():
    from tests import test_region_cell_count_gpu as gpu

    for sequence_name, alphabet, kinds, region_name in gpu.EXAMPLE_CASES:
        region = (gpu.MAIN_REGIONS if alphabet == "nuc" else gpu.S_REGIONS)[region_name]
        value = gpu.example_value(sequence_name, alphabet, kinds, region)
        for at_least, at_most in gpu.region_bounds(value):
            assert _cuts(gpu.mask_for(value, at_least, at_most)), (sequence_name, kinds, region_name, at_least, at_most)
    assert len(gpu.example_symbols(None, "nuc")[1]) == gpu.MAIN_POSITIONS and len(gpu.example_symbols("S", "aa")[1]) == gpu.S_POSITIONS
    # the fixed thresholds of the composition, Mutations, batch, shortcut and whole-sequence tests
    spike, gene_e = gpu.example_value(None, "nuc", "missing", gpu.MAIN_REGIONS["S"]), gpu.example_value(None, "nuc", "missing", gpu.MAIN_REGIONS["E"])
    for mask in (spike == 0, gpu.example_value("S", "aa", "substitutions", gpu.S_REGIONS["RBD"]) >= 3, gene_e == 0,
                 gpu.example_value(None, "nuc", ["substitutions", "deletions"], gpu.MAIN_REGIONS["241"]) >= 1,
                 gpu.example_value(None, "nuc", "deletions", gpu.MAIN_REGIONS["S"]) > 0, gpu.example_value(None, "nuc", "missing", (1, 100)) >= 1,
                 gpu.example_value(None, "nuc", "missing", (29804, gpu.MAIN_POSITIONS)) >= 1, whole.values(gpu.example_table(None, "nuc"), whole.MISSING) <= 100):
        assert _cuts(mask)
    assert gpu.MAIN_REGIONS["E"][1] - gpu.MAIN_REGIONS["E"][0] + 1 == 228 and int(gene_e.max()) < 228


def test_every_action_has_a_region_that_cuts():
    from tests import test_region_cell_count_gpu as gpu

    rows = np.ones(100, dtype=bool)
    value_of = lambda kinds, name=None, alphabet="nuc": (lambda first, last: gpu.example_value(name, alphabet, kinds, (first, last)))  # noqa: E731
    names = [region[0] for region in gpu.action_regions()]
    assert len(set(names)) == len(names) == 21 and names != sorted(names)
    counts = gpu.action_counts(gpu.action_regions(), value_of("missing"), rows, None, 0)
    own = [count for count, region in zip(counts, gpu.action_regions()) if region[3] is not None]
    assert any(0 < count < 100 for count in own) and any(0 < count < 100 for count in set(counts) - set(own)) and len(set(counts)) > 4
    counts = gpu.action_counts(gpu.many_regions(), value_of(["missing", "deletions"]), rows, 1, None)
    assert len(counts) == 256 and any(0 < count < 100 for count in counts) and len(set(counts)) > 3
    s_regions = [(name, first, last, None, None) for name, (first, last) in gpu.S_REGIONS.items()]
    assert any(0 < count < 100 for count in gpu.action_counts(s_regions, value_of(["substitutions", "deletions"], "S", "aa"), rows, 1, 20))


def test_the_synthetic_thresholds_and_actions_cut():
    from tests import test_region_cell_count_gpu as gpu
    from tests.test_mutations_over_time_gpu import N_ROWS, _synthetic_dates, _synthetic_matrix

    rng = np.random.default_rng(2026)  # the fixture `synthetic` of tests/test_distance_matrix_gpu.py
    sym = _synthetic_matrix(rng)
    _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    cases = list(gpu.synthetic_cases(sym))
    assert {tuple(region) for _, region, _, _ in cases} == set(gpu.SYNTHETIC_REGIONS) and len(cases) >= 40
    for kinds, region, at_least, at_most in cases:
        assert _cuts(gpu.mask_for(gpu.synthetic_value(sym, kinds, region), at_least, at_most)), (kinds, region, at_least, at_most)
    for kinds in ("missing", ["substitutions", "ambiguous"]):
        for rows in (np.ones(N_ROWS, dtype=bool), bucket < 100):
            counts = gpu.action_counts(gpu.SYNTHETIC_ACTION, lambda first, last: gpu.synthetic_value(sym, kinds, (first, last)), rows, 1, None)
            assert sum(0 < count < int(rows.sum()) for count in counts) >= 3, (kinds, counts)


def test_the_kernel_fixtures_hold_what_their_tests_take_them_for():
    from tests import test_region_cell_values_gpu as kernels
    from tests.test_grouped_kernels_gpu import _matrix
    from tests.test_row_hashes_gpu import runs_matrix

    for alphabet in ("nuc", "aa"):
        sym = _matrix(alphabet)
        for name, ranges in kernels.RANGE_SETS.items():  # every kind occurs in every range set
            assert (ref.region_cells(sym, sym[0], alphabet, ranges).reshape(-1, 4).max(axis=0) > 0).all(), (alphabet, name)
    sym = runs_matrix()
    eight = ref.values(sym, sym[0], "nuc", kernels.RUN_RANGE_SETS["eight"], whole.MISSING)
    assert (eight[:, 14] == 5).all() and eight[:, 18].tolist() == [4, 5, 5, 5, 5, 5, 5, 4] and eight[:, 10].tolist() == [5, 2, 0, 0, 0, 0, 0, 0]
    inside = ref.values(sym, sym[0], "nuc", kernels.RUN_RANGE_SETS["inside-runs"], whole.MISSING)
    assert inside[:, 10].tolist() == [4, 1, 0, 0] and inside[:, 12].tolist() == [0, 0, 2, 4] and inside[:, 4000].tolist() == [1, 2, 0, 0]
    wide = kernels.wide_matrix()
    cells = ref.region_cells(wide, wide[0], "nuc", [(22, 278)])
    assert (cells[0].max(axis=0) > 0).all() and cells[0][129].tolist() == [0, 0, 256, 0]
