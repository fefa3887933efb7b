"""silo_gpu_row_hashes and silo_gpu_store_row_hashes (K20, csrc/silo_gpu_distinct.hip) called directly, against the numpy statement
of tests/distinct_reference.py: every layout a finalized store can have, in both alphabets, the row counts around a word, null
genomes, runs of the missing symbol at the ends of a row and over a whole one, the characters silo_gpu_reconstruct_sequences gives
for the same rows (the rule of who claims a cell), the kept copy and the refusals.  Every comparison is an exact equality."""
import ctypes
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import distinct_reference as ref  # noqa: E402
from tests.test_grouped_kernels_gpu import LAYOUT_IDS, LAYOUTS, N_ROWS, _assert_layout, _layout_store, _matrix  # noqa: E402
from tests.test_kernels_gpu import AA_CHARS, NUC_CHARS, make_store, random_symbols  # noqa: E402

FILL = 0xA5
FILLED = np.uint64(0xA5A5A5A5A5A5A5A5)
ROW_COUNTS = [1, 63, 64, 65, 2049]
IDENTITY_POSITIONS = 37


def _chars(alphabet):
    return NUC_CHARS if alphabet == "nuc" else AA_CHARS


@functools.lru_cache(maxsize=None)
def identity_matrix(n):
    """Random symbols, every one of the alphabet: the store keeps its build-time planes at this length."""
    sym = random_symbols(np.random.default_rng(900 + n), n, IDENTITY_POSITIONS, "nuc")
    if n > 3:
        sym[n - 1] = sym[0]
        sym[n // 2] = sym[0]
    sym.setflags(write=False)
    return sym


@functools.lru_cache(maxsize=None)
def null_genome_matrix():
    """(symbols as the store holds them, is_null): 300 rows of which every seventh has no genome — the missing symbol throughout."""
    rng = np.random.default_rng(77)
    sym = random_symbols(rng, 300, 29, "nuc")
    is_null = (np.arange(300) % 7 == 3).astype(np.uint8)
    effective = sym.copy()
    effective[is_null.astype(bool)] = 15
    effective.setflags(write=False)
    return sym, is_null, effective


@functools.lru_cache(maxsize=None)
def runs_matrix():
    """5 000 rows x 40 positions, nearly all rows the reference, with runs of N that begin at position 0, that end at the last
    position, that cover a whole row, single cells at both ends and rows that differ from a neighbour only inside a run."""
    rng = np.random.default_rng(78)
    reference = rng.integers(1, 5, size=40).astype(np.uint8)
    sym = np.tile(reference, (5000, 1))
    mutated = rng.choice(5000, size=400, replace=False)
    sym[mutated, rng.integers(0, 40, size=400)] = rng.integers(0, 5, size=400)
    sym[10, :7] = 15
    sym[11, :1] = 15
    sym[12, 33:] = 15
    sym[13, 39:] = 15
    sym[14, :] = 15
    sym[15, :] = 15
    sym[16, :20] = 15
    sym[16, 20:] = 15
    sym[17, 0] = 15
    sym[17, 39] = 15
    sym[18, 1:39] = 15
    sym[4000:4100, 5:9] = 15
    sym[4100:4200, 5:10] = 15
    sym.setflags(write=False)
    return sym


def _symbols_of_chars(chars, alphabet):
    table = np.full(256, 255, dtype=np.uint8)
    table[_chars(alphabet)] = np.arange(len(_chars(alphabet)), dtype=np.uint8)
    table[ord("?")] = ref.NO_SYMBOL
    sym = table[chars]
    assert (sym != 255).all()
    return sym


def _reconstructed(store, n):
    return np.concatenate([store.reconstruct_sequences(0, np.arange(begin, min(n, begin + 60_000))) for begin in range(0, n, 60_000)])


def _check_table(store, sym, context):
    """The table of a store against numpy on the symbol matrix: every real row, (0, 0) for the padding rows, the guard rows
    untouched."""
    n = len(sym)
    got = store.row_hashes(0, fill=FILL, guard_rows=3)
    padded = store.row_words * 64
    assert got.shape == (padded + 3, 2)
    assert np.array_equal(got[:n], ref.row_hashes(sym)), context
    assert not got[n:padded].any(), context
    assert (got[padded:] == FILLED).all(), context
    return got[:n]


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("knob4,knob8", LAYOUTS, ids=LAYOUT_IDS)
def test_every_layout_matches_numpy(built, alphabet, knob4, knob8):
    sym = _matrix(alphabet)
    with _layout_store(alphabet, knob4, knob8) as store:
        _assert_layout(store, alphabet, knob4, knob8)
        _check_table(store, sym, (alphabet, knob4, knob8))
        if alphabet == "nuc":  # the claim rule: what the hashes count is what silo_gpu_reconstruct_sequences writes
            assert np.array_equal(_symbols_of_chars(_reconstructed(store, N_ROWS), alphabet), sym)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_on_identity_planes(built, n):
    sym = identity_matrix(n)
    with make_store(n, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        assert store.scan_escapes(0) == 0
        hashes = _check_table(store, sym, n)
        if n > 3:
            assert np.array_equal(hashes[n - 1], hashes[0]) and np.array_equal(hashes[n // 2], hashes[0])


def test_null_genomes(built):
    sym, is_null, effective = null_genome_matrix()
    with make_store(len(sym), [dict(name="s", alphabet="nuc", reference=np.ones(sym.shape[1], dtype=np.uint8))]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym], is_null)
        store.finalize()
        assert np.array_equal(_symbols_of_chars(_reconstructed(store, len(sym)), "nuc"), effective)
        hashes = _check_table(store, effective, "null genomes")
        null_rows = np.flatnonzero(is_null)
        assert len(null_rows) > 10 and (hashes[null_rows] == hashes[null_rows[0]]).all()


@pytest.mark.parametrize("knob4,knob8", [(0, 0), (0, -1), (-1, 0)], ids=["derived", "missing-plane", "identity"])
def test_runs_at_the_ends_of_a_row_and_over_a_whole_row(built, knob4, knob8):
    sym = runs_matrix()
    store = make_store(len(sym), [dict(name="s", alphabet="nuc", reference=sym[0].copy())])
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
    with store:
        if knob8 != 0:
            assert store.scan_runs(0) == 0 and store.plane(0, 0, 15) is not None
        assert np.array_equal(_symbols_of_chars(_reconstructed(store, len(sym)), "nuc"), sym)
        hashes = _check_table(store, sym, (knob4, knob8))
        assert np.array_equal(hashes[14], hashes[15]) and np.array_equal(hashes[14], hashes[16])
        assert not np.array_equal(hashes[4000], hashes[4100])


def test_the_kept_copy(built):
    sym = _matrix("nuc")
    with _layout_store("nuc", 0, 0) as store:
        cells = store.row_words * 64 * 2
        before = store.device_bytes
        direct = store.row_hashes(0, fill=FILL)
        assert store.device_bytes == before  # silo_gpu_row_hashes keeps nothing
        pointers = [None] * 8
        barrier = threading.Barrier(8)

        def first_call(index):
            barrier.wait()
            pointers[index] = store.kept_row_hashes(0)

        threads = [threading.Thread(target=first_call, args=(index,)) for index in range(8)]
        for thread in threads:
            thread.start()
        for thread in threads:
            thread.join()
        assert pointers[0] and len(set(pointers)) == 1
        assert store.device_bytes == before + 8 * cells
        assert store.kept_row_hashes(0) == pointers[0] and store.kept_row_hashes(0) == pointers[0]
        assert store.device_bytes == before + 8 * cells
        kept = store.read(ctypes.c_void_p(pointers[0]), np.uint64, cells).reshape(-1, 2)
        assert np.array_equal(kept, direct) and np.array_equal(kept[:N_ROWS], ref.row_hashes(sym))


def test_refusals_leave_the_output_alone(built):
    from silo_amd import binding

    sym = identity_matrix(65)
    lib = binding.load_library()
    with make_store(65, [dict(name="s", alphabet="nuc", reference=sym[0].copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        rows = store.row_words * 64
        table = store.malloc(16 * rows)
        scratch = store.malloc(binding.row_hash_scratch_bytes(IDENTITY_POSITIONS))
        kept = ctypes.c_void_p()
        try:
            store.memset(table, FILL, 16 * rows)
            # not finalized yet
            assert lib.silo_gpu_row_hashes(store.handle, 0, table, scratch, None) != 0
            assert lib.silo_gpu_store_row_hashes(store.handle, 0, ctypes.byref(kept), None) != 0 and not kept.value
            store.finalize()
            before = store.device_bytes
            assert lib.silo_gpu_row_hashes(None, 0, table, scratch, None) != 0
            assert lib.silo_gpu_row_hashes(store.handle, 1, table, scratch, None) != 0
            assert lib.silo_gpu_row_hashes(store.handle, 0, None, scratch, None) != 0
            assert lib.silo_gpu_row_hashes(store.handle, 0, table, None, None) != 0
            assert lib.silo_gpu_store_row_hashes(None, 0, ctypes.byref(kept), None) != 0
            assert lib.silo_gpu_store_row_hashes(store.handle, 1, ctypes.byref(kept), None) != 0
            assert lib.silo_gpu_store_row_hashes(store.handle, 0, None, None) != 0
            assert not kept.value and store.device_bytes == before
            store.synchronize()
            assert (store.read(table, np.uint64, 2 * rows) == FILLED).all()
            assert lib.silo_gpu_row_hashes(store.handle, 0, table, scratch, None) == 0
            store.synchronize()
            assert np.array_equal(store.read(table, np.uint64, 2 * rows).reshape(-1, 2)[:65], ref.row_hashes(sym))
        finally:
            store.free(table)
            store.free(scratch)
