"""A store gives back every byte of device memory it took: create, build, finalize, one Mutations scan, destroy, over and over,
with the free bytes of the device read through a second, tiny store that stays alive.  One-pass build, two-pass build, and a
two-pass build abandoned between its passes (destroyed after build_pass(2), never finalized)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

N, POSITIONS = 70_001, 200  # rows of more than one column tile: finalize re-encodes; a second, partial slice of 2^17 rows


@pytest.fixture(scope="module")
def model(built):
    from silo_amd import synth

    tree = synth.make_lineage_tree(40)
    lineage = synth.assign_lineages(N, tree, 2024)
    reference = synth.random_reference(POSITIONS, "nuc", 17)
    return reference, synth.make_model(N, reference, "nuc", tree, lineage, seed=99, store_index=0)


def free_bytes(store):
    free, total = ctypes.c_uint64(), ctypes.c_uint64()
    assert store.lib.silo_gpu_store_memory_info(store.handle, ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def cycle(model, mode):
    from silo_amd.binding import GpuStore

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


@pytest.mark.parametrize("mode", ["one_pass", "two_pass", "abandoned"])
def test_the_free_bytes_come_back_after_every_cycle(model, mode):
    from silo_amd.binding import GpuStore

    reference, _ = model
    with GpuStore(64, [dict(name="witness", alphabet="nuc", reference=reference.copy())]) as witness:
        cycle(model, mode)  # warm-up: the per-thread pools and side streams exist from here on
        after = []
        for _ in range(3):
            cycle(model, mode)
            after.append(free_bytes(witness))
        print(mode, "free bytes after each cycle", after)
        assert after[2] == after[0]
