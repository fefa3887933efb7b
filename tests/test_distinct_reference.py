"""The numpy statement of DistinctSequences (tests/distinct_reference.py) against the known answers of its definition, the host
function of the library (silo_gpu_row_hash_term, which needs no device), the constants of the binding against the header, and —
on every symbol matrix the GPU tests use — the representatives by hash against the representatives by exact equality of rows: the
check, on the CPU, that no fixture holds a collision.  Runs anywhere."""
import os
import re

import numpy as np
import pytest

from tests import distinct_reference as ref
from tests import sample_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_known_answers():
    assert [int(ref.terms([p], [s], lane)[0]) for p, s in ((0, 0), (29902, 15), (1273, 31)) for lane in (0, 1)] == [
        0xE220A8397B1DCDAF, 0x1FDD7128F310C389, 0x267055D5DFCB477C, 0x6AE0021E344CED32, 0xBADDF521CAAC5267, 0xBB9A4FB1C805E7EF]
    for position, symbol in ((0, 0), (29902, 15), (1273, 31), (2 ** 23, 24)):  # the scalar splitmix64 of the Sample reference
        x = position * 32 + symbol
        assert int(ref.terms([position], [symbol], 0)[0]) == sample_reference.splitmix64(x)
        assert int(ref.terms([position], [symbol], 1)[0]) == sample_reference.splitmix64(x + 2 ** 40)
    sym = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 4], [3, 2, 1], [1, 2, ref.NO_SYMBOL]])
    hashes = ref.row_hashes(sym)
    assert hashes[0].tolist() == [18436898564895704466, 15246863189105014066] and hashes[2].tolist() == [2254887826969688728, 11864493668406112736]
    assert hashes[0, 0] == (sample_reference.splitmix64(1) + sample_reference.splitmix64(34) + sample_reference.splitmix64(67)) % 2 ** 64
    assert ref.select(sym, [1, 1, 1, 1, 1]).tolist() == [True, False, True, True, True]
    assert ref.select(sym, [0, 1, 1, 1, 0]).tolist() == [False, True, True, True, False]
    assert not ref.select(sym, [0, 0, 0, 0, 0]).any()
    # a permutation of a row's symbols over positions is another row: the position is part of the term
    assert len(np.unique(ref.row_hashes(np.array([[1, 2], [2, 1], [1, 1], [2, 2]])), axis=0)) == 4


def test_the_library_computes_the_same_terms(built):
    from silo_amd import binding

    for position in (0, 1, 47, 29902, 2 ** 23 - 1, 2 ** 27 - 1):
        for symbol in (0, 4, 15, 24, 31):
            for lane in (0, 1):
                assert binding.row_hash_term(position, symbol, lane) == int(ref.terms([position], [symbol], lane)[0]), (position, symbol, lane)


def test_the_constants_of_the_binding_are_the_headers():
    from silo_amd import binding

    header = open(os.path.join(ROOT, "include", "silo_gpu.h")).read()
    assert int(re.search(r"#define SILO_GPU_ROW_HASH_NO_SYMBOL (\d+)u", header).group(1)) == binding.ROW_HASH_NO_SYMBOL == ref.NO_SYMBOL
    assert int(re.search(r"#define SILO_GPU_DISTINCT_EMPTY (0x[0-9A-F]+)u", header).group(1), 16) == binding.DISTINCT_EMPTY
    assert "#define SILO_GPU_ROW_HASH_SCRATCH_BYTES(positions) ((size_t)(positions) * 17u + 1024u)" in header
    assert "#define SILO_GPU_DISTINCT_TABLE_BYTES(slots) (((size_t)(slots) + 1u) * 4u)" in header
    assert binding.row_hash_scratch_bytes(29903) == 29903 * 17 + 1024 and binding.distinct_table_bytes(1 << 20) == ((1 << 20) + 1) * 4
    assert binding.DISTINCT_PART_DTYPE.itemsize == 24 and binding.DISTINCT_PART_DTYPE.names == ("hashes_dev", "first_row", "sequence_count", "row_words", "reserved")
    struct = re.search(r"typedef struct silo_gpu_distinct_part \{(.*?)\} silo_gpu_distinct_part;", header, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == list(binding.DISTINCT_PART_DTYPE.names)
    assert [binding.distinct_slots(rows) for rows in (0, 1, 2, 3, 64, 65, 70_001)] == [2, 2, 4, 8, 128, 256, 262144]


def _classes(sym):
    _, class_of_row = np.unique(sym, axis=0, return_inverse=True)
    return np.bincount(class_of_row.reshape(-1))


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_the_layout_matrices_hold_classes_of_several_rows_and_rows_that_are_alone(alphabet):
    from tests.test_grouped_kernels_gpu import _matrix

    sizes = _classes(_matrix(alphabet))
    assert (sizes > 1).sum() > 0 and (sizes == 1).sum() > 0


def _fixtures():
    from tests import test_distinct_gpu, test_row_hashes_gpu
    from tests.test_distance_matrix_gpu import N_ROWS
    from tests.test_grouped_kernels_gpu import _matrix
    from tests.test_mutations_over_time_gpu import _synthetic_matrix

    yield "layouts nuc", _matrix("nuc")
    yield "layouts aa", _matrix("aa")
    for n in test_row_hashes_gpu.ROW_COUNTS:
        yield f"identity {n}", test_row_hashes_gpu.identity_matrix(n)
    yield "null genomes", test_row_hashes_gpu.null_genome_matrix()[2]
    yield "runs", test_row_hashes_gpu.runs_matrix()
    yield "planted main", test_distinct_gpu.planted_symbols(None)
    yield "planted S", test_distinct_gpu.planted_symbols("S")
    synthetic = _synthetic_matrix(np.random.default_rng(2026))  # the matrix of the fixture `synthetic` of tests/test_distance_matrix_gpu.py
    assert synthetic.shape[0] == N_ROWS
    yield "synthetic", synthetic


def test_no_fixture_of_the_gpu_tests_holds_a_collision():
    rng = np.random.default_rng(1)
    seen = 0
    for name, sym in _fixtures():
        n = len(sym)
        for selected in (np.ones(n, dtype=bool), rng.random(n) < 0.5, np.arange(n) >= n // 3):
            by_hash = ref.select_by_hash(ref.row_hashes(sym), selected)
            assert np.array_equal(by_hash, ref.select_by_equality(sym, selected)), name
            assert by_hash.sum() == len(np.unique(sym[selected], axis=0)) and not (by_hash & ~selected).any(), name
        seen += 1
    assert seen == 12


def test_the_planted_copies_are_what_the_gpu_test_takes_them_for():
    from tests import test_distinct_gpu as planted

    sym = planted.planted_symbols(None)
    n = len(sym)
    want = ref.select(sym, np.ones(n, dtype=bool))
    assert want[planted.ORIGINAL] and want[planted.OTHER] and not want[planted.COPIES].any() and not want[planted.LONE_COPY]
    assert want[planted.WITH_N] and want[planted.WITH_CODE]
    assert (sym[planted.WITH_N] != sym[planted.ORIGINAL]).sum() == 1 and (sym[planted.WITH_CODE] != sym[planted.ORIGINAL]).sum() == 1
    assert 15 in sym[planted.WITH_N][sym[planted.WITH_N] != sym[planted.ORIGINAL]] and sym[planted.WITH_CODE][sym[planted.WITH_CODE] != sym[planted.ORIGINAL]][0] in (5, 6)
