"""A store gives back every byte of device memory it took: create, build, finalize, one Mutations scan, destroy, over and over,
with the free bytes of the device read through a second, tiny store that stays alive.  One-pass build, two-pass build, and a
two-pass build abandoned between its passes (destroyed after build_pass(2), never finalized); a store appended in two batches
and read back through the calls that allocate for themselves (FastaAligned, planes of single symbols, membership tables, the
hashed group count and its refusal); a store imported from roaring payloads.  Everything a cycle reads is compared with numpy."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402
from tests import roaring_payloads as rp  # noqa: E402

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
MISSING = 15

N, POSITIONS = 70_001, 200  # rows of more than one column tile: finalize re-encodes; a second, partial slice of 2^17 rows


@pytest.fixture(scope="module")
def model(built):
    from silo_amd import synth

    tree = synth.make_lineage_tree(40)
    lineage = synth.assign_lineages(N, tree, 2024)
    reference = synth.random_reference(POSITIONS, "nuc", 17)
    return reference, synth.make_model(N, reference, "nuc", tree, lineage, seed=99, store_index=0)


@pytest.fixture(scope="module")
def alignment():
    """Symbol ids [N][POSITIONS] with ambiguity codes (sparse keys) and runs of the missing symbol, the null genomes of the second
    batch, and what the store then holds (a null genome is the missing symbol everywhere)."""
    rng = np.random.default_rng(70_001)
    reference = rng.integers(1, 5, size=POSITIONS).astype(np.uint8)
    sym = np.where(rng.random((N, POSITIONS)) < 0.97, reference, rng.integers(0, 5, size=(N, POSITIONS))).astype(np.uint8)
    ambiguous = rng.random((N, POSITIONS)) < 0.002
    sym[ambiguous] = rng.integers(5, 15, size=int(ambiguous.sum()))
    for row in np.nonzero(rng.random(N) < 0.02)[0].tolist():
        start = int(rng.integers(0, POSITIONS - 1))
        sym[row, start:start + int(rng.integers(1, 30))] = MISSING
    is_null = np.zeros(N, dtype=np.uint8)
    is_null[APPEND_CUT:] = rng.random(N - APPEND_CUT) < 0.01
    stored = sym.copy()
    stored[is_null.astype(bool)] = MISSING
    return reference, sym, is_null, stored


APPEND_CUT = 20_001  # the second batch is the larger one: both staging buffers are allocated again for it


def free_bytes(store):
    free, total = ctypes.c_uint64(), ctypes.c_uint64()
    assert store.lib.silo_gpu_store_memory_info(store.handle, ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def appended_cycle(alignment):
    from silo_amd.binding import GpuStore, SiloGpuError

    reference, sym, is_null, stored = alignment
    rng = np.random.default_rng(3)
    with GpuStore(N, [dict(name="main", alphabet="nuc", reference=reference.copy())]) as store:
        store.append_sequences(0, 0, NUC_CHARS[sym[:APPEND_CUT]])
        store.append_sequences(0, APPEND_CUT, NUC_CHARS[sym[APPEND_CUT:]], is_null[APPEND_CUT:].copy())
        store.finalize()
        rows = np.concatenate([[0, APPEND_CUT - 1, APPEND_CUT, N - 1], np.nonzero(is_null)[0][:3], rng.choice(N, size=20, replace=False)]).astype(np.uint32)
        assert np.array_equal(store.reconstruct_sequences(0, rows), NUC_CHARS[stored[rows]])
        bitset = store.bitset_alloc()
        for position, symbol in ((7, int(reference[7])), (100, 1 + int(reference[100]) % 4), (150, MISSING)):
            store.sparse_plane(0, position, symbol, bitset)
            want = dense.pack_bits(stored[:, position] == symbol)
            got = store.bitset_download(bitset)
            assert np.array_equal(got[: len(want)], want) and not got[len(want):].any(), (position, symbol)
        ids = (np.arange(N, dtype=np.uint32) * 7919) % 11
        membership = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1], dtype=np.uint8)
        ids_dev = store.upload_column(ids)
        store.bitset_from_value_ids(bitset, ids_dev, membership)
        want = dense.pack_bits(membership[ids] != 0)
        assert np.array_equal(store.bitset_download(bitset)[: len(want)], want)
        pair_rows = np.sort(rng.choice(N, size=5000, replace=False)).astype(np.uint32)
        pair_ids = rng.integers(0, 11, size=5000).astype(np.uint32)
        rows_dev, pair_ids_dev = store.upload_column(pair_rows), store.upload_column(pair_ids)
        store.bitset_from_pairs(bitset, rows_dev, pair_ids_dev, len(pair_rows), membership)
        member_rows = np.zeros(N, bool)
        member_rows[pair_rows[membership[pair_ids] != 0]] = True
        want = dense.pack_bits(member_rows)
        assert np.array_equal(store.bitset_download(bitset)[: len(want)], want)
        column = (np.arange(N, dtype=np.uint32) * 31) % 5000
        column_dev = store.upload_column(column)
        want_ids, want_counts = np.unique(column.astype(np.uint64) * 11 + ids, return_counts=True)
        got_ids, got_counts = store.group_count_hashed(None, [column_dev, ids_dev], [5000, 11], N)
        assert np.array_equal(got_ids, want_ids) and np.array_equal(got_counts, want_counts.astype(np.uint32))
        with pytest.raises(SiloGpuError):  # max_rows understated: the call frees all five of its arrays
            store.group_count_hashed(None, [column_dev, ids_dev], [5000, 11], 100)
        for pointer in (ids_dev, rows_dev, pair_ids_dev, column_dev, bitset):
            store.free(pointer)


def imported_cycle():
    from silo_amd import binding

    case = rp.import_case("n65537-aa")
    with binding.GpuStore(case.n, [case.store_description()]) as store:
        binding.import_missing_rows(store.handle, 0, 0, list(rp.case_missing_rows(case.name, True)))
        for position, (bitmaps, flipped, deleted) in enumerate(rp.case_payloads(case.name, "plain", True)):
            binding.import_position(store.handle, 0, position, bitmaps, flipped, deleted)
        store.finalize()
        want = dense.mutation_counts(case.sym, np.ones(case.n, bool), list(store.scan_symbols[0]))
        assert np.array_equal(store.mutations_scan(0), want)


def cycle(model, mode, alignment=None):
    from silo_amd.binding import GpuStore

    if mode == "appended":
        return appended_cycle(alignment)
    if mode == "imported":
        return imported_cycle()
    reference, synth_model = model
    with GpuStore(N, [dict(name="main", alphabet="nuc", reference=reference.copy())]) as store:
        if mode != "one_pass":
            store.build_pass(0, 1)
            store.generate_synthetic(0, synth_model)
            store.build_pass(0, 2)
            assert store.build_mode(0) == 2  # the encoding pass: the layout in the making is allocated
            if mode == "abandoned":
                return
        store.generate_synthetic(0, synth_model)
        store.finalize()
        assert store.scan_escapes(0) > 0 and store.scan_runs(0) > 0  # adaptive planes, keys, runs: every stage of finalize ran
        store.mutations_scan(0)


@pytest.mark.parametrize("mode", ["one_pass", "two_pass", "abandoned", "appended", "imported"])
def test_the_free_bytes_come_back_after_every_cycle(model, alignment, mode):
    from silo_amd.binding import GpuStore

    reference, _ = model
    with GpuStore(64, [dict(name="witness", alphabet="nuc", reference=reference.copy())]) as witness:
        cycle(model, mode, alignment)  # warm-up: the per-thread pools and side streams exist from here on
        after = []
        for _ in range(3):
            cycle(model, mode, alignment)
            after.append(free_bytes(witness))
        print(mode, "free bytes after each cycle", after)
        assert after[2] == after[0]
