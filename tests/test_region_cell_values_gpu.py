"""silo_gpu_region_cell_values (K23, csrc/silo_gpu_region_counts.hip) called directly, against the numpy statement of
tests/region_counts_reference.py: every layout a finalized store can have, in both alphabets and under every kinds mask, with range
sets that are the whole sequence, single positions at both ends, neighbours that touch, ranges with gaps around them and one range
per position; the row counts around a word, null genomes, runs of the missing symbol that begin and end inside and outside ranges,
a reference symbol that is not valid, 256 regions at once, the whole-sequence region against K22's table, and the refusals.  Every
comparison is an exact equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cell_counts_reference as whole  # noqa: E402
from tests import region_counts_reference as ref  # noqa: E402
from tests.test_grouped_kernels_gpu import LAYOUT_IDS, LAYOUTS, N_ROWS, POSITIONS, _assert_layout, _layout_store, _matrix  # noqa: E402
from tests.test_kernels_gpu import NUC_CHARS, make_store  # noqa: E402
from tests.test_row_cell_counts_gpu import _store_with_runs, invalid_reference  # noqa: E402
from tests.test_row_hashes_gpu import IDENTITY_POSITIONS, ROW_COUNTS, identity_matrix, null_genome_matrix, runs_matrix  # noqa: E402

FILL = 0xA5
FILLED = np.uint32(0xA5A5A5A5)
GUARD = 5
MASKS = list(range(1, 16))
RANGE_SETS = {  # on the 24 positions of tests/test_grouped_kernels_gpu.py
    "whole": [(0, POSITIONS)],
    "first": [(0, 1)],
    "last": [(POSITIONS - 1, POSITIONS)],
    "touching": [(0, 5), (5, 6), (6, POSITIONS)],
    "gaps": [(3, 4), (10, 17)],
    "singles": [(p, p + 1) for p in range(POSITIONS)],
}
RUN_RANGE_SETS = {  # on the 40 positions of runs_matrix(): runs are [0,7) [0,1) [33,40) [39,40) [0,40) [1,39) [5,9) [5,10) and two single cells
    "inside-runs": [(2, 6), (6, 8), (20, 35), (36, 40)],
    "eight": [(0, 5), (5, 10), (10, 15), (15, 20), (20, 25), (25, 30), (30, 35), (35, 40)],
    "ends": [(0, 1), (39, 40)],
    "between": [(10, 30)],
    "whole": [(0, 40)],
}


def check_values(store, sym, reference, alphabet, ranges, masks, context, cells=None):
    """The columns of a store against numpy on the symbol matrix: every real row, zeros for the padding rows, the guard untouched."""
    n = len(sym)
    padded = store.row_words * 64
    cells = ref.region_cells(sym, reference, alphabet, ranges) if cells is None else cells
    for mask in masks:
        got = store.region_cell_values(0, ranges, mask, fill=FILL, guard_rows=GUARD)
        assert got.shape == (len(ranges) * padded + GUARD,)
        columns = got[:len(ranges) * padded].reshape(len(ranges), padded)
        want = ref.values_of_cells(cells, mask)
        assert np.array_equal(columns[:, :n], want), (context, ranges, mask)
        assert not columns[:, n:].any(), (context, ranges, mask)
        assert (got[len(ranges) * padded:] == FILLED).all(), (context, ranges, mask)


@functools.lru_cache(maxsize=None)
def _layout_cells(alphabet, name):
    sym = _matrix(alphabet)
    return ref.region_cells(sym, sym[0], alphabet, RANGE_SETS[name])


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("knob4,knob8", LAYOUTS, ids=LAYOUT_IDS)
def test_every_layout_mask_and_range_set_matches_numpy(built, alphabet, knob4, knob8):
    sym = _matrix(alphabet)
    with _layout_store(alphabet, knob4, knob8) as store:
        _assert_layout(store, alphabet, knob4, knob8)
        for name, ranges in RANGE_SETS.items():
            check_values(store, sym, sym[0], alphabet, ranges, MASKS, (alphabet, knob4, knob8, name), _layout_cells(alphabet, name))


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_the_whole_sequence_region_is_the_table_of_row_cell_counts(built, alphabet):
    with _layout_store(alphabet, 0, 0) as store:
        table = store.row_cell_counts(0, fill=FILL)
        padded = store.row_words * 64
        for mask in MASKS:
            got = store.region_cell_values(0, [(0, POSITIONS)], mask, fill=FILL)
            assert np.array_equal(got[:padded].astype(np.uint64), whole.values(table[:padded], mask)), mask
        assert whole.values(table[:N_ROWS], 15).max() > 0


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_on_identity_planes(built, n):
    sym = identity_matrix(n)
    with make_store(n, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_escapes(0) == 0
        for ranges in ([(0, IDENTITY_POSITIONS)], [(0, 1), (1, 20), (36, 37)], [(p, p + 1) for p in range(IDENTITY_POSITIONS)]):
            check_values(store, sym, sym[0], "nuc", ranges, (1, 4, 8, 15), n)


def test_null_genomes(built):
    sym, is_null, effective = null_genome_matrix()
    reference = np.ones(sym.shape[1], dtype=np.uint8)
    with make_store(len(sym), [dict(name="s", alphabet="nuc", reference=reference)]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym], is_null)
        store.finalize()
        ranges = [(0, 3), (4, 5), (10, 29)]
        check_values(store, effective, reference, "nuc", ranges, MASKS, "null genomes")
        got = store.region_cell_values(0, ranges, whole.MISSING).reshape(len(ranges), -1)
        null_rows = np.flatnonzero(is_null)
        assert len(null_rows) > 10 and (got[:, null_rows] == np.array([[3], [1], [19]])).all()  # MISSING throughout


@pytest.mark.parametrize("knob4,knob8", [(0, 0), (0, -1), (-1, 0)], ids=["derived", "missing-plane", "identity"])
def test_ranges_that_begin_and_end_inside_runs(built, knob4, knob8):
    sym = runs_matrix()
    with _store_with_runs(sym, sym[0], knob4, knob8) as store:
        if knob8 != 0:
            assert store.scan_runs(0) == 0 and store.plane(0, 0, 15) is not None
        for name, ranges in RUN_RANGE_SETS.items():
            check_values(store, sym, sym[0], "nuc", ranges, (1, 2, 4, 5, 11, 15), (knob4, knob8, name))
        eight = store.region_cell_values(0, RUN_RANGE_SETS["eight"], whole.MISSING).reshape(8, -1)
        assert (eight[:, 14] == 5).all() and (eight[:, 15] == 5).all()  # a row missing throughout touches every region
        assert eight[:, 18].tolist() == [4, 5, 5, 5, 5, 5, 5, 4] and eight[:, 10].tolist() == [5, 2, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("knob4,knob8", [(0, 0), (-1, 0)], ids=["derived", "identity"])
def test_a_reference_symbol_that_is_not_valid(built, knob4, knob8):
    sym, reference = invalid_reference()
    with _store_with_runs(sym, reference, knob4, knob8) as store:
        for ranges in ([(0, 1), (7, 8), (20, 21), (39, 40)], [(0, 8), (8, 40)], [(0, 40)]):
            check_values(store, sym, reference, "nuc", ranges, MASKS, (knob4, knob8))
        got = store.region_cell_values(0, [(0, 1), (7, 8), (20, 21), (39, 40)], whole.SUBSTITUTIONS).reshape(4, -1)
        assert got[:, 0].tolist() == [1, 1, 1, 1]  # the row the reference was made from: a substitution wherever it is not valid


@functools.lru_cache(maxsize=None)
def wide_matrix():
    """130 rows x 300 positions: mostly the reference, with substitutions, deletions, ambiguity codes, runs of N and a row that is
    missing throughout — three row words' worth of lanes under 256 regions."""
    rng = np.random.default_rng(2300)
    reference = rng.integers(1, 5, size=300).astype(np.uint8)
    sym = np.tile(reference, (130, 1))
    cells = rng.choice(130 * 300, size=4000, replace=False)
    sym.reshape(-1)[cells] = rng.integers(0, 16, size=len(cells))
    for row in range(5, 130, 9):
        start = int(rng.integers(0, 290))
        sym[row, start:start + int(rng.integers(2, 60))] = 15
    sym[129, :] = 15
    sym[0] = reference
    sym.setflags(write=False)
    return sym


@pytest.mark.parametrize("knob4,knob8", [(-1, 0), (0, 0)], ids=["identity", "derived"])
def test_256_single_position_regions(built, knob4, knob8):
    sym = wide_matrix()
    ranges = [(p, p + 1) for p in range(22, 22 + ref.MAX_REGIONS)]
    with _store_with_runs(sym, sym[0], knob4, knob8) as store:
        check_values(store, sym, sym[0], "nuc", ranges, (3, 4, 8, 15), (knob4, knob8))
        check_values(store, sym, sym[0], "nuc", [(0, 22), (22, 150), (151, 300)], MASKS, (knob4, knob8))


def test_refusals_leave_the_output_alone(built):
    from silo_amd import binding

    sym = identity_matrix(65)
    lib = binding.load_library()
    with make_store(65, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        cells = store.row_words * 64 * 2
        columns = store.malloc(4 * cells)
        scratch = store.malloc(binding.region_value_scratch_bytes(IDENTITY_POSITIONS))
        P = IDENTITY_POSITIONS

        def call(ranges, mask=15, handle=store.handle, seqstore=0, out=columns, work=scratch, n=None, null_ranges=False):
            array = np.ascontiguousarray(ranges, dtype=np.uint32).reshape(-1, 2)
            pointer = None if null_ranges else array.ctypes.data_as(binding.ctypes.c_void_p)
            return lib.silo_gpu_region_cell_values(handle, seqstore, pointer, len(array) if n is None else n, mask, out, work, None)

        try:
            store.memset(columns, FILL, 4 * cells)
            good = [(0, 3), (3, P)]
            assert call(good) != 0  # not finalized yet
            store.finalize()
            before = store.device_bytes
            assert call(good, handle=None) != 0 and call(good, seqstore=1) != 0 and call(good, out=None) != 0 and call(good, work=None) != 0
            assert call(good, null_ranges=True) != 0
            assert call(good, n=0) != 0 and call([(0, 1)] * (ref.MAX_REGIONS + 1), n=ref.MAX_REGIONS + 1) != 0
            assert call([(3, 3)]) != 0 and call([(4, 3)]) != 0               # empty
            assert call([(5, 9), (0, 3)]) != 0                               # out of order
            assert call([(0, 5), (4, 9)]) != 0 and call([(0, 5), (0, 5)]) != 0  # overlapping
            assert call([(0, P + 1)]) != 0 and call([(P, P + 1)]) != 0      # past the end
            assert call(good, mask=0) != 0 and call(good, mask=16) != 0
            store.synchronize()
            assert (store.read(columns, np.uint32, cells) == FILLED).all() and store.device_bytes == before
            assert call(good) == 0
            store.synchronize()
            got = store.read(columns, np.uint32, cells).reshape(2, -1)
            assert np.array_equal(got[:, :65], ref.values(sym, sym[0], "nuc", good, 15)) and not got[:, 65:].any()
            assert store.device_bytes == before  # nothing is kept by the store
        finally:
            store.free(columns)
            store.free(scratch)
