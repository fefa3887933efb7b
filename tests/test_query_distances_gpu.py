"""silo_gpu_query_distances (K11, csrc/silo_gpu_nearest.hip) called directly, against the numpy reference of
tests/nearest_rows_reference.py (pinned without a GPU by tests/test_nearest_rows_reference.py): every cell of every row, the
padding rows included, in every store layout and both alphabets; the row counts around a word and a block; more positions than a
vertical counter holds; the refusals.  The output is filled with 0xA5 before every call.  Every comparison is an exact integer
equality."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import nearest_rows_reference as ref  # noqa: E402
from tests.pair_distances_reference import AA_VALID, NUC_VALID  # noqa: E402
from tests.test_grouped_kernels_gpu import (ABSENT_AT, LAYOUT_IDS, LAYOUTS, N_ROWS, POSITIONS, SETTLED, _alphabet, _assert_layout, _layout_store,  # noqa: E402
                                            _matrix)
from tests.test_kernels_gpu import AA_CHARS, NUC_CHARS, make_store, random_symbols  # noqa: E402

FILL = 0xA5
VALID = {"nuc": NUC_VALID, "aa": AA_VALID}
CHARS = {"nuc": NUC_CHARS, "aa": AA_CHARS}


def _check(store, chars, query, valid, what):
    """Every cell of the table: the rows of the store against numpy, the padding rows (0, 0)."""
    n = len(chars)
    got = store.query_distances(0, query, fill=FILL)
    assert got.shape == (store.row_words * 64, 2) and got.dtype == np.uint32
    want = ref.query_distances(chars, query, valid)
    wrong = np.flatnonzero((got[:n] != want).any(axis=1))
    assert len(wrong) == 0, (what, wrong[:5], got[wrong[:5]], want[wrong[:5]])
    assert not got[n:].any(), what
    return got


def _queries(alphabet):
    """(name, characters) for the layout stores: rows of the store and constructed queries."""
    table = _alphabet(alphabet)
    sym = _matrix(alphabet)
    chars = CHARS[alphabet]
    valid = np.array(sorted(table.valid_mutation_symbols))
    is_valid = np.isin(sym, valid)
    ambiguity = ~is_valid & (sym != table.missing)
    counts = np.stack([np.bincount(sym[:, p], minlength=table.count) for p in range(POSITIONS)])  # [P][symbols]
    valid_counts = counts[:, valid]
    order = np.argsort(-valid_counts, axis=1, kind="stable")
    dominant = valid[order[:, 0]].astype(np.uint8)
    second = valid[order[:, 1]].astype(np.uint8)

    partly_missing = (sym == table.missing).any(axis=1) & is_valid.any(axis=1)
    in_run = int(np.flatnonzero(partly_missing)[0])
    with_code = int(np.flatnonzero(ambiguity.any(axis=1) & ~partly_missing)[0])
    # a symbol that is rare at a settled position: neither the derived symbol nor a one-hot row — an escape key
    settled = SETTLED[2]
    rare = [s for s in valid if 0 < counts[settled, s] < N_ROWS // 1000]
    assert rare
    with_escape = int(np.flatnonzero(sym[:, settled] == rare[0])[0])
    absent = [s for s in valid if counts[ABSENT_AT, s] == 0]
    assert absent
    unseen = dominant.copy()
    unseen[ABSENT_AT] = absent[0]
    odd = chars[dominant].copy()
    odd[1], odd[SETTLED[0]], odd[POSITIONS - 1] = ord("a"), ord("?"), 0
    return [
        ("row in a run of the missing symbol", chars[sym[in_run]]),
        ("row with an ambiguity code", chars[sym[with_code]]),
        ("row with an escape-key symbol", chars[sym[with_escape]]),
        ("dominant symbols", chars[dominant]),
        ("second symbols", chars[second]),
        ("a symbol no row has", chars[unseen]),
        ("all missing", np.full(POSITIONS, chars[table.missing], dtype=np.uint8)),
        ("a, ? and NUL", odd),
    ]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_every_cell_in_every_layout(built, layout, alphabet):
    """The 70 001 x 24 stores of tests/test_grouped_kernels_gpu.py: derived symbols with runs of the missing symbol, one-hot rows,
    code planes with escape keys, identity planes, the missing symbol in a plane of its own."""
    sym = _matrix(alphabet)
    chars = CHARS[alphabet][sym]
    with _layout_store(alphabet, *layout) as store:
        _assert_layout(store, alphabet, *layout)
        for name, query in _queries(alphabet):
            got = _check(store, chars, query, VALID[alphabet], (LAYOUT_IDS[LAYOUTS.index(layout)], alphabet, name))
            if name == "all missing":
                assert not got.any()
            if name == "dominant symbols":
                assert got[:N_ROWS, 1].max() == POSITIONS and 0 < got[:N_ROWS, 0].max()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_row_count_edges_on_identity_planes(built, n):
    """Short rows: the store keeps its build-time identity planes (no code map, no keys)."""
    rng = np.random.default_rng(900 + n)
    sym = random_symbols(rng, n, 24, "nuc")
    chars = NUC_CHARS[sym]
    with make_store(n, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, chars)
        store.finalize()
        assert store.scan_escapes(0) == 0
        for name, query in (("first row", chars[0]), ("last row", chars[n - 1]), ("random", NUC_CHARS[random_symbols(rng, 1, 24, "nuc")[0]]),
                            ("all N", np.full(24, ord("N"), np.uint8))):
            _check(store, chars, query, NUC_VALID, (n, name))


def test_more_positions_than_a_vertical_counter_holds(built):
    """A counter of the plane pass has QUERY_DISTANCE_COUNTER_PLANES = 12 bit planes: it holds 4 095 adds, and a thread walks
    chunks of at least 4 096 positions.  With 4 200 positions where the query differs from every row, the first chunk adds 4 096
    times to every row's distance and compared counters: a counter that was not unpacked in time would read 0."""
    from silo_amd import binding

    width = binding.QUERY_DISTANCE_COUNTER_PLANES
    n, positions = 130, 4200
    assert positions > (1 << width) > positions // 2
    rng = np.random.default_rng(12)
    sym = np.full((n, positions), 1, dtype=np.uint8)  # A
    sym[rng.random((n, positions)) < 0.01] = 15        # a few N
    chars = NUC_CHARS[sym]
    with make_store(n, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.tune(4, -1)  # identity planes: every position adds its rows to the compared and the distance counter
        try:
            store.append_sequences(0, 0, chars)
            store.finalize()
        finally:
            store.tune(4, 0)
        assert store.scan_escapes(0) == 0
        got = _check(store, chars, np.full(positions, ord("C"), np.uint8), NUC_VALID, "all C")
        assert got[:n, 0].min() > (1 << width) and np.array_equal(got[:n, 0], got[:n, 1])
        _check(store, chars, np.full(positions, ord("A"), np.uint8), NUC_VALID, "all A")


def test_refusals_write_nothing(built):
    from silo_amd.binding import SiloGpuError, query_distance_scratch_bytes

    rng = np.random.default_rng(5)
    sym = random_symbols(rng, 100, 24, "nuc")
    query = NUC_CHARS[sym[0]]
    with make_store(100, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        cells = store.row_words * 64 * 2
        out = store.malloc(cells * 4)
        scratch = store.malloc(query_distance_scratch_bytes(24))
        store.memset(out, FILL, cells * 4)
        with pytest.raises(SiloGpuError):
            store.query_distances(1, query, out_ptr=out, scratch_ptr=scratch)  # seqstore id out of range
        with pytest.raises(SiloGpuError):
            store.query_distances(0, None, out_ptr=out, scratch_ptr=scratch)
        with pytest.raises(SiloGpuError):
            store.query_distances(0, query, out_ptr=out, scratch_ptr=None)
        with pytest.raises(SiloGpuError):
            store.query_distances(0, query, out_ptr=ctypes.c_void_p(None), scratch_ptr=scratch)
        lib = store.lib
        assert lib.silo_gpu_query_distances(None, 0, query.ctypes.data_as(ctypes.c_void_p), out, scratch, None) != 0
        store.synchronize()
        assert (store.read(out, np.uint8, cells * 4) == FILL).all()
        store.query_distances(0, query, out_ptr=out, scratch_ptr=scratch)  # the same buffers serve a good call
        got = store.read(out, np.uint32, cells).reshape(-1, 2)
        assert np.array_equal(got[:100], ref.query_distances(NUC_CHARS[sym], query, NUC_VALID)) and not got[100:].any()
    with make_store(10, [dict(name="s", alphabet="nuc", reference=np.ones(24, dtype=np.uint8))]) as empty:  # no sequences yet
        out = empty.malloc(4096 * 8)
        empty.memset(out, FILL, 4096 * 8)
        with pytest.raises(SiloGpuError):
            empty.query_distances(0, query, out_ptr=out)
        empty.synchronize()
        assert (empty.read(out, np.uint8, 4096 * 8) == FILL).all()
