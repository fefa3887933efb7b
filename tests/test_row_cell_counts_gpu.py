"""silo_gpu_row_cell_counts and silo_gpu_store_row_cell_counts (K22, csrc/silo_gpu_cell_counts.hip) called directly, against the numpy
statement of tests/cell_counts_reference.py: every layout a finalized store can have, in both alphabets, the row counts around a
word, null genomes, runs of the missing symbol at the ends of a row and over a whole one, a reference symbol that is not valid, the
stats silo_gpu_sequence_differences (K18) reports for the characters silo_gpu_reconstruct_sequences gives for the same rows, the kept
copy and the refusals.  Every comparison is an exact equality."""
import ctypes
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cell_counts_reference as ref  # noqa: E402
from tests.test_grouped_kernels_gpu import LAYOUT_IDS, LAYOUTS, N_ROWS, _assert_layout, _layout_store, _matrix  # noqa: E402
from tests.test_kernels_gpu import AA_CHARS, NUC_CHARS, make_store  # noqa: E402
from tests.test_row_hashes_gpu import IDENTITY_POSITIONS, ROW_COUNTS, identity_matrix, null_genome_matrix, runs_matrix  # noqa: E402

FILL = 0xA5
FILLED = np.uint32(0xA5A5A5A5)
INVALID_REFERENCE_AT = (0, 7, 20, 39)  # positions of runs_matrix() whose reference symbol is replaced by N, R, N, Y


def _chars(alphabet):
    return NUC_CHARS if alphabet == "nuc" else AA_CHARS


def _check_table(store, sym, reference, alphabet, context):
    """The table of a store against numpy on the symbol matrix: every real row, zeros for the padding rows, the guard rows
    untouched."""
    n = len(sym)
    got = store.row_cell_counts(0, fill=FILL, guard_rows=3)
    padded = store.row_words * 64
    assert got.shape == (padded + 3, 4)
    assert np.array_equal(got[:n], ref.cells(sym, reference, alphabet)), context
    assert not got[n:padded].any(), context
    assert (got[padded:] == FILLED).all(), context
    return got[:n]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("knob4,knob8", LAYOUTS, ids=LAYOUT_IDS)
def test_every_layout_matches_numpy(built, alphabet, knob4, knob8):
    sym = _matrix(alphabet)
    with _layout_store(alphabet, knob4, knob8) as store:
        _assert_layout(store, alphabet, knob4, knob8)
        cells = _check_table(store, sym, sym[0], alphabet, (alphabet, knob4, knob8))
        assert (cells.max(axis=0) > 0).all() and (cells[:, 2] == sym.shape[1]).sum() >= 100  # every kind occurs; rows missing throughout


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_on_identity_planes(built, n):
    sym = identity_matrix(n)
    with make_store(n, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_escapes(0) == 0
        cells = _check_table(store, sym, sym[0], "nuc", n)
        assert cells[0, 0] == 0 and cells[0, 1] == 0  # a row is no substitution or deletion against itself


def test_null_genomes(built):
    sym, is_null, effective = null_genome_matrix()
    reference = np.ones(sym.shape[1], dtype=np.uint8)
    with make_store(len(sym), [dict(name="s", alphabet="nuc", reference=reference)]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym], is_null)
        store.finalize()
        cells = _check_table(store, effective, reference, "nuc", "null genomes")
        null_rows = np.flatnonzero(is_null)
        assert len(null_rows) > 10 and (cells[null_rows] == (0, 0, sym.shape[1], 0)).all()


def _store_with_runs(sym, reference, knob4, knob8):
    store = make_store(len(sym), [dict(name="s", alphabet="nuc", reference=reference.copy())])
    store.tune(4, knob4)
    store.tune(8, knob8)
    store.tune(9, -1)
    try:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
    finally:
        store.tune(4, 0)
        store.tune(8, 0)
        store.tune(9, 0)
    return store


@pytest.mark.parametrize("knob4,knob8", [(0, 0), (0, -1), (-1, 0)], ids=["derived", "missing-plane", "identity"])
def test_runs_at_the_ends_of_a_row_and_over_a_whole_row(built, knob4, knob8):
    sym = runs_matrix()
    with _store_with_runs(sym, sym[0], knob4, knob8) as store:
        if knob8 != 0:
            assert store.scan_runs(0) == 0 and store.plane(0, 0, 15) is not None
        cells = _check_table(store, sym, sym[0], "nuc", (knob4, knob8))
        assert cells[14, 2] == 40 and cells[16, 2] == 40 and cells[10, 2] == 7 and cells[13, 2] == 1 and cells[17, 2] == 2 and cells[18, 2] == 38


@functools.lru_cache(maxsize=None)
def invalid_reference():
    """The reference of runs_matrix() with N and ambiguity codes at four positions, the first and the last among them: every valid
    symbol there is a substitution or a deletion, an N is still missing, and a row's own code is ambiguous, not SAME."""
    sym = runs_matrix().copy()
    reference = sym[0].copy()
    reference[list(INVALID_REFERENCE_AT)] = (15, 5, 15, 6)
    sym[20, 7] = 5   # the reference's own ambiguity code
    sym[21, 39] = 0  # a deletion where the reference is not valid
    sym.setflags(write=False)
    reference.setflags(write=False)
    return sym, reference


@pytest.mark.parametrize("knob4,knob8", [(0, 0), (-1, 0)], ids=["derived", "identity"])
def test_a_reference_symbol_that_is_not_valid(built, knob4, knob8):
    sym, reference = invalid_reference()
    with _store_with_runs(sym, reference, knob4, knob8) as store:
        cells = _check_table(store, sym, reference, "nuc", (knob4, knob8))
        assert cells[0, 0] == len(INVALID_REFERENCE_AT)  # the row the reference was made from: substitutions where it is not valid
        assert cells[14].tolist() == [0, 0, 40, 0] and cells[20, 3] == 1 and cells[21, 1] >= 1


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_equal_to_the_stats_of_sequence_differences(built, alphabet):
    """The definition: for every row the four numbers K18 reports for the row's reconstructed characters (9 000 rows, derived layout)."""
    from silo_amd import binding

    sym = _matrix(alphabet)
    rows = np.arange(61_000, 70_000)
    with _layout_store(alphabet, 0, 0) as store:
        cells = store.row_cell_counts(0, fill=FILL)[:N_ROWS]
        chars = store.reconstruct_sequences(0, rows)
    _, stats, _, status = binding.sequence_differences(alphabet, chars, _chars(alphabet)[sym[0]], 0)
    assert status == 0
    stats = stats[:len(rows) * 4].reshape(-1, 4)
    assert np.array_equal(cells[rows], stats)
    assert (stats.max(axis=0) > 0).all()
    assert np.array_equal(ref.symbols_of_chars(chars, alphabet), sym[rows])  # the claim rule: what is counted is what is reconstructed


def test_the_kept_copy(built):
    sym = _matrix("nuc")
    with _layout_store("nuc", 0, 0) as store:
        cells = store.row_words * 64 * 4
        before = store.device_bytes
        direct = store.row_cell_counts(0, fill=FILL)
        assert store.device_bytes == before  # silo_gpu_row_cell_counts keeps nothing
        pointers = [None] * 8
        barrier = threading.Barrier(8)

        def first_call(index):
            barrier.wait()
            pointers[index] = store.kept_row_cell_counts(0)

        threads = [threading.Thread(target=first_call, args=(index,)) for index in range(8)]
        for thread in threads:
            thread.start()
        for thread in threads:
            thread.join()
        assert pointers[0] and len(set(pointers)) == 1
        assert store.device_bytes == before + 4 * cells
        assert store.kept_row_cell_counts(0) == pointers[0] and store.kept_row_cell_counts(0) == pointers[0]
        assert store.device_bytes == before + 4 * cells
        kept = store.read(ctypes.c_void_p(pointers[0]), np.uint32, cells).reshape(-1, 4)
        assert np.array_equal(kept, direct) and np.array_equal(kept[:N_ROWS], ref.cells(sym, sym[0], "nuc"))


def test_refusals_leave_the_output_alone(built):
    from silo_amd import binding

    sym = identity_matrix(65)
    lib = binding.load_library()
    with make_store(65, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        rows = store.row_words * 64
        table = store.malloc(16 * rows)
        scratch = store.malloc(binding.row_cell_count_scratch_bytes(IDENTITY_POSITIONS))
        kept = ctypes.c_void_p()
        try:
            store.memset(table, FILL, 16 * rows)
            # not finalized yet
            assert lib.silo_gpu_row_cell_counts(store.handle, 0, table, scratch, None) != 0
            assert lib.silo_gpu_store_row_cell_counts(store.handle, 0, ctypes.byref(kept), None) != 0 and not kept.value
            store.finalize()
            before = store.device_bytes
            assert lib.silo_gpu_row_cell_counts(None, 0, table, scratch, None) != 0
            assert lib.silo_gpu_row_cell_counts(store.handle, 1, table, scratch, None) != 0
            assert lib.silo_gpu_row_cell_counts(store.handle, 0, None, scratch, None) != 0
            assert lib.silo_gpu_row_cell_counts(store.handle, 0, table, None, None) != 0
            assert lib.silo_gpu_store_row_cell_counts(None, 0, ctypes.byref(kept), None) != 0
            assert lib.silo_gpu_store_row_cell_counts(store.handle, 1, ctypes.byref(kept), None) != 0
            assert lib.silo_gpu_store_row_cell_counts(store.handle, 0, None, None) != 0
            assert not kept.value and store.device_bytes == before
            store.synchronize()
            assert (store.read(table, np.uint32, 4 * rows) == FILLED).all()
            assert lib.silo_gpu_row_cell_counts(store.handle, 0, table, scratch, None) == 0
            store.synchronize()
            assert np.array_equal(store.read(table, np.uint32, 4 * rows).reshape(-1, 4)[:65], ref.cells(sym, sym[0], "nuc"))
        finally:
            store.free(table)
            store.free(scratch)
