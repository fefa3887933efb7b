"""The numpy statement of K22 (tests/cell_counts_reference.py) against a plain loop over characters and against the per-row stats of
tests/sequence_differences_reference.py on the example data set, the constants of the binding against the header, and — on the CPU —
the guard that keeps the GPU tests from being vacuous: every threshold they ask for selects a row and leaves a row out on its
fixture, every binning gives at least two non-empty bins, and the fixtures hold what the tests take them for."""
import os
import re

import numpy as np
import pytest

from tests import cell_counts_reference as ref
from tests import sequence_differences_reference as differences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cells_by_loop(rows, reference, alphabet):
    """The rule of the module's docstring, character by character."""
    out = np.zeros((len(rows), 4), dtype=np.uint32)
    missing = "N" if alphabet == "nuc" else "X"
    for r, row in enumerate(rows):
        for c, at_reference in zip(row, reference):
            if c == missing:
                out[r, 2] += 1
            elif c not in ref.VALID[alphabet]:
                out[r, 3] += 1
            elif c == at_reference:
                pass
            elif c == "-":
                out[r, 1] += 1
            else:
                out[r, 0] += 1
    return out


def _sym(rows, alphabet):
    return np.array([[ref.CHARS[alphabet].index(c) for c in row] for row in rows], dtype=np.uint8)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_numpy_matches_a_character_loop(alphabet):
    rng = np.random.default_rng(5)
    chars = ref.CHARS[alphabet]
    rows = ["".join(rng.choice(list(chars), size=60)) for _ in range(200)]
    rows.append(chars[-1] * 60)
    rows.append("-" * 60)
    for reference in ("".join(rng.choice(list(ref.VALID[alphabet][1:]), size=60)), "".join(rng.choice(list(chars), size=60))):  # the second: symbols that are not valid
        got = ref.cells(_sym(rows, alphabet), _sym([reference], alphabet)[0], alphabet)
        assert np.array_equal(got, _cells_by_loop(rows, reference, alphabet))
        assert (got.sum(axis=1) <= 60).all() and (got.max(axis=0) > 0).all()
        assert got[-2].tolist() == [0, 0, 60, 0]
    no_symbol = np.full((1, 5), ref.NO_SYMBOL, dtype=np.uint8)
    assert ref.cells(no_symbol, np.ones(5, dtype=np.uint8), alphabet).tolist() == [[0, 0, 0, 5]]


def test_values_selection_and_bins():
    table = np.array([[1, 2, 3, 4], [0, 0, 0, 0], [0xFFFFFFFF] * 4, [5, 0, 7, 0], [9, 9, 9, 9]], dtype=np.uint32)
    assert ref.values(table, 15).tolist() == [10, 0, 4 * 0xFFFFFFFF, 12, 36] and ref.values(table, 5).tolist() == [4, 0, 2 * 0xFFFFFFFF, 12, 18]
    assert ref.mask_of("missing") == 4 and ref.mask_of(["ambiguous", "substitutions"]) == 9 and ref.mask_of(list(ref.KINDS)) == 15
    assert ref.selected(table, 4, 15, 1, 12).tolist() == [True, False, False, True, False]
    assert ref.selected(table, 5, 15).tolist() == [True, True, False, True, True]
    assert not ref.selected(table, 5, 15, 3, 2).any()
    assert ref.bins(table, [1, 1, 1, 1, 0], 15, 5, 4).tolist() == [1, 0, 2, 1]
    assert ref.response_rows(np.array([1, 0, 2, 1], dtype=np.uint64), 5) == [
        {"from": 0, "to": 4, "count": 1}, {"from": 10, "to": 14, "count": 2}, {"from": 15, "to": None, "count": 1}]


def test_example_dataset_matches_the_stats_of_sequence_differences():
    from tests import dataset
    from tests.test_cell_count_gpu import example_table

    data = dataset.load_example_dataset()
    for sequence_name, alphabet, rows, reference in ((None, "nuc", data["nuc"]["main"], data["nuc_references"]["main"]),
                                                     ("S", "aa", data["aa"]["S"], data["aa_references"]["S"])):
        assert all(row is not None for row in rows)
        canonical = [row.replace(".", "-").replace("U", "T") if alphabet == "nuc" else row for row in rows]
        chars = np.array([list(row.encode()) for row in canonical], dtype=np.uint8)
        _, stats, _ = differences.difference_records(chars, reference, alphabet)
        assert np.array_equal(example_table(sequence_name, alphabet), stats)


def test_the_constants_of_the_binding_are_the_headers():
    from silo_amd import binding

    header = open(os.path.join(ROOT, "include", "silo_gpu.h")).read()
    assert int(re.search(r"#define SILO_GPU_CELL_COUNT_KINDS (\d+)", header).group(1)) == binding.CELL_COUNT_KINDS == len(ref.KINDS)
    assert int(re.search(r"#define SILO_GPU_MAX_CELL_COUNT_BINS (\d+)", header).group(1)) == binding.MAX_CELL_COUNT_BINS == ref.MAX_BINS
    for name, bit, kind in (("SUBSTITUTIONS", binding.CELL_COUNT_SUBSTITUTIONS, "substitutions"), ("DELETIONS", binding.CELL_COUNT_DELETIONS, "deletions"),
                            ("MISSING", binding.CELL_COUNT_MISSING, "missing"), ("AMBIGUOUS", binding.CELL_COUNT_AMBIGUOUS, "ambiguous")):
        assert int(re.search(r"#define SILO_GPU_CELL_COUNT_%s (\d+)u" % name, header).group(1)) == bit == ref.mask_of(kind)
    assert "#define SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(positions) ((size_t)(positions) * 17u + 1024u)" in header
    assert binding.row_cell_count_scratch_bytes(29903) == 29903 * 17 + 1024
    for entry in ("silo_gpu_row_cell_counts", "silo_gpu_store_row_cell_counts", "silo_gpu_bitset_from_cell_counts", "silo_gpu_cell_count_histogram"):
        assert entry in binding.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % entry, header)
    assert (ref.SUBSTITUTIONS, ref.DELETIONS, ref.MISSING, ref.AMBIGUOUS) == (1, 2, 4, 8)
    assert differences.STATS == len(ref.KINDS)  # K18's stats order


# ---- the guard: no threshold or binning of the GPU tests is vacuous on its fixture ----------------------------------------------
def _cuts(value, at_least, at_most):
    from tests.test_cell_count_gpu import mask_for

    mask = mask_for(value, at_least, at_most)
    return 0 < int(mask.sum()) < len(mask)


def test_every_json_threshold_cuts_its_fixture():
    from tests import test_cell_count_gpu as gpu

    for cases, table_of in ((gpu.EXAMPLE_CASES, gpu.example_table), (gpu.PLANTED_CASES, gpu.planted_table)):
        for sequence_name, alphabet, kinds in cases:
            table = table_of(sequence_name, alphabet)
            for kind in ([kinds] if isinstance(kinds, str) else kinds):  # no kind is constant on the fixture it is used on
                assert len(np.unique(ref.values(table, ref.mask_of(kind)))) > 1, (sequence_name, kind)
            value = ref.values(table, ref.mask_of(kinds))
            for at_least, at_most in gpu.bounds_for(value):
                assert _cuts(value, at_least, at_most), (sequence_name, kinds, at_least, at_most)
    assert len(np.unique(gpu.example_table("S", "aa")[:, 3])) == 1  # why S is not used for "ambiguous": the kind is constant there
    ambiguous = gpu.planted_table("S", "aa")[:, 3]
    assert {row: int(ambiguous[row]) for row in np.flatnonzero(ambiguous)} == gpu.PLANTED_CODES
    # the fixed thresholds of the composition, Mutations, batch and shortcut tests
    main, gene = gpu.example_table(None, "nuc"), gpu.example_table("S", "aa")
    for value, at_least, at_most in ((main[:, 2], None, 100), (ref.values(gene, 3), 10, None), (gene[:, 0], 10, None), (ref.values(main, 12), 1, 50),
                                     (main[:, 1], None, 30), (gene[:, 2], None, 0)):
        assert _cuts(value, at_least, at_most), (at_least, at_most)


def test_every_json_binning_gives_two_bins():
    from tests import test_cell_count_gpu as gpu

    for binnings, table_of in ((gpu.EXAMPLE_BINNINGS, gpu.example_table), (gpu.PLANTED_BINNINGS, gpu.planted_table)):
        for sequence_name, alphabet, kinds, bin_width, max_bins in binnings:
            table = table_of(sequence_name, alphabet)
            histogram = ref.bins(table, np.ones(len(table), dtype=bool), ref.mask_of(kinds), bin_width, max_bins or 1024)
            assert (histogram > 0).sum() >= 2, (sequence_name, kinds, bin_width, max_bins)
    main = gpu.example_table(None, "nuc")
    assert ref.bins(main, np.ones(len(main), dtype=bool), ref.MISSING, 100, 8)[[0, 7]].all()  # the first bin and the open last one
    assert (ref.bins(main, np.ones(len(main), dtype=bool), ref.SUBSTITUTIONS, 2, 1024) > 0).sum() > 8


def test_the_synthetic_thresholds_and_binnings_cut():
    from tests import test_cell_count_gpu as gpu
    from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS, _synthetic_dates, _synthetic_matrix

    rng = np.random.default_rng(2026)  # the fixture `synthetic` of tests/test_distance_matrix_gpu.py
    sym = _synthetic_matrix(rng)
    _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    table = gpu.synthetic_table(sym)
    assert table.shape == (N_ROWS, 4)
    for kinds in gpu.SYNTHETIC_KINDS:
        value = ref.values(table, ref.mask_of(kinds))
        for at_least, at_most in gpu.bounds_for(value)[:3]:
            assert _cuts(value, at_least, at_most), (kinds, at_least, at_most)
    for kinds, bin_width, max_bins in gpu.SYNTHETIC_BINNINGS:
        for rows in (np.ones(N_ROWS, dtype=bool), bucket < 100):
            assert (ref.bins(table, rows, ref.mask_of(kinds), bin_width, max_bins or 1024) > 0).sum() >= 2
    assert (table[:, 2] == POSITIONS).sum() > 100


def test_the_kernel_fixtures_hold_what_their_tests_take_them_for():
    from tests import test_bitset_from_cell_counts_gpu as bitset
    from tests import test_cell_count_histogram_gpu as histogram
    from tests import test_row_cell_counts_gpu as rows
    from tests.test_grouped_kernels_gpu import _matrix
    from tests.test_row_hashes_gpu import runs_matrix

    for alphabet in ("nuc", "aa"):
        sym = _matrix(alphabet)
        cells = ref.cells(sym, sym[0], alphabet)
        assert (cells.max(axis=0) > 0).all() and (cells[:, 2] == sym.shape[1]).sum() >= 100
        assert (cells[61_000:70_000].max(axis=0) > 0).all()
    sym = runs_matrix()
    cells = ref.cells(sym, sym[0], "nuc")
    assert cells[14, 2] == 40 and cells[16, 2] == 40 and cells[10, 2] == 7 and cells[13, 2] == 1 and cells[17, 2] == 2 and cells[18, 2] == 38
    sym, reference = rows.invalid_reference()
    cells = ref.cells(sym, reference, "nuc")
    assert cells[0, 0] == len(rows.INVALID_REFERENCE_AT) and cells[14].tolist() == [0, 0, 40, 0] and cells[20, 3] == 1 and cells[21, 1] >= 1
    assert not np.array_equal(cells, ref.cells(sym, runs_matrix()[0], "nuc"))
    n = 70_001
    table = bitset.make_table(n, bitset.row_words_of(n, True))
    for mask in bitset.MASKS:
        counts = [int(ref.selected(table, n, mask, at_least, at_most).sum()) for at_least, at_most in bitset.bounds_of(table, n, mask)]
        assert counts[0] == n and 0 < counts[1] < n and 0 < counts[2] < n and 0 < counts[3] < counts[1], mask
        assert counts[8] == 0 and counts[10] == 0 and counts[11] == 0 and counts[7] > 0, mask
    for mask, at_least, at_most in ((4, 0, 0), (1, 7, 20), (15, 30, 200), (5, 10, 150)):
        assert 0 < int(ref.selected(table, n, mask, at_least, at_most).sum()) < n
    assert int(ref.values(table[:n], histogram.MASK).max()) <= histogram.LARGEST
    assert (ref.bins(table, np.arange(len(table)) < n, histogram.MASK, 7, 256) > 0).sum() > 40
