"""The count slot, the row slot, the value-id bitset and the insertion-pair kernels through the C ABI, each against numpy.

These entry points serve every product query (operators.cpp, database.cpp, metadata_actions.cpp) and are reached by the
other test files only through the engine on the 100-row example data set: one tile, one block, one part, a few dozen pairs.
Here they get the sizes where their block counts, strides, epochs, re-arming and atomics matter.  Every comparison is an
exact integer or bit equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402
from tests.test_kernels_gpu import (  # noqa: E402
    MUTATIONS_SELECT_PROPORTIONS,
    _eval,
    filter_eval_programs,
    make_store,
    mutations_select_expected,
    mutations_select_table,
)

REFERENCE = np.ones(4, dtype=np.uint8)
EVAL_ROWS = [1, 63, 64, 777,          # one tile, mostly inactive lanes
             8191, 8192, 8193,        # one 128-word tile, exactly and just past it
             65_537,                  # 9 tiles: more tiles than the 8 waves of a fat block
             300_001, 1_200_003]      # many blocks
N_WIDE_LEAVES = 19                    # an n-ary run over more than 16 leaves: 8 + 8 + 3 and 16 + 3 loads
TUNE_EVAL_LEAF_BATCH = 2              # SILO_GPU_TUNE_EVAL_LEAF_BATCH


def _plain_store(n):
    return make_store(n, [dict(name="s", alphabet="nuc", reference=REFERENCE)])


def _upload_masks(store, masks):
    leaves = []
    for mask in masks:
        ptr = store.bitset_alloc()
        store.bitset_upload(ptr, dense.pack_bits(mask))
        leaves.append(ptr)
    return leaves


def _eval_masks(rng, n):
    """Leaves 0..4 as in test_filter_eval_ops; leaves 5..23: a run of sparse ones (its union stays far from all rows); leaves
    24..42: a run of dense ones (its intersection stays far from none)."""
    masks = [rng.random(n) < p for p in (0.5, 0.2, 0.7, 0.05, 0.9)]
    masks += [rng.random(n) < 0.03 for _ in range(N_WIDE_LEAVES)]
    masks += [rng.random(n) < 0.97 for _ in range(N_WIDE_LEAVES)]
    return masks


def _count_slot_programs(masks):
    """(code, n_slots, expected mask): the programs of test_filter_eval_ops, programs whose value travels through the highest
    slots of launches with 12, 16, 17 and 32 slots (16: the last with 8 waves per block, 17: the first with 4, 32:
    SILO_GPU_MAX_SLOTS), and n-ary runs over more than 16 leaves."""
    from silo_amd import binding as b

    L = b.LEAF_OPERAND
    programs = list(filter_eval_programs(masks[:5]))
    total5 = sum(m.astype(int) for m in masks[:5])
    for n_slots in (12, 16, 17, 32):
        top = n_slots - 1
        programs.append((b.encode(b.OP_MOV, top, L + 4) + b.encode(b.OP_NOT, top - 1, top) + b.encode(b.OP_OR, 0, top - 1, L + 1), n_slots,
                         ~masks[4] | masks[1]))
        # a 3-bit counter in the three highest slots
        code = b.encode(b.OP_ZERO, top - 2) + b.encode(b.OP_ZERO, top - 1) + b.encode(b.OP_ZERO, top)
        code += b.encode(b.OP_CNT_ADD_N, top - 2, 0, 3, imm=0 | (5 << 16)) + b.encode(b.OP_CNT_GE, 0, top - 2, 3, imm=2)
        programs.append((code, n_slots, total5 >= 2))
    sparse_run, dense_run = masks[5:5 + N_WIDE_LEAVES], masks[5 + N_WIDE_LEAVES:5 + 2 * N_WIDE_LEAVES]
    programs.append((b.encode(b.OP_OR_N, 0, imm=5 | (N_WIDE_LEAVES << 16)), 1, np.logical_or.reduce(sparse_run)))
    programs.append((b.encode(b.OP_AND_N, 0, imm=(5 + N_WIDE_LEAVES) | (N_WIDE_LEAVES << 16)), 1, np.logical_and.reduce(dense_run)))
    zero5 = []
    for slot in range(1, 6):
        zero5 += b.encode(b.OP_ZERO, slot)
    total_sparse = sum(m.astype(int) for m in sparse_run)
    programs.append((zero5 + b.encode(b.OP_CNT_ADD_N, 1, 0, 5, imm=5 | (N_WIDE_LEAVES << 16)) + b.encode(b.OP_CNT_GE, 0, 1, 5, imm=2), 6,
                     total_sparse >= 2))
    programs.append((zero5 + b.encode(b.OP_CNT_ADD_NOT_N, 1, 0, 5, imm=5 | (N_WIDE_LEAVES << 16)) + b.encode(b.OP_CNT_EQ, 0, 1, 5, imm=N_WIDE_LEAVES - 1),
                     6, (N_WIDE_LEAVES - total_sparse) == N_WIDE_LEAVES - 1))
    return programs


def _check_count_slot_programs(n):
    from silo_amd.binding import CountSlot

    rng = np.random.default_rng(1000 + n)
    masks = _eval_masks(rng, n)
    with _plain_store(n) as store:
        leaves = _upload_masks(store, masks)
        out = store.bitset_alloc()
        slot = CountSlot()
        try:
            for index, (code, n_slots, want) in enumerate(_count_slot_programs(masks)):
                reference_words, reference_count = _eval(store, code, leaves, n_slots)  # silo_gpu_filter_eval
                assert reference_count == int(want.sum()), index
                # with an output bitset: the destination starts out as all ones, so every word the kernel owes is seen
                store.memset(out, 0xFF, store.row_words * 8)
                store.filter_eval_count(code, leaves, n_slots, slot, out)
                assert slot.wait() == int(want.sum()), (index, n_slots)
                words = store.bitset_download(out)
                bits = dense.unpack_bits(words, store.row_words * 64)
                assert np.array_equal(bits[:n], want), (index, n_slots)
                assert not bits[n:].any(), (index, n_slots)
                assert np.array_equal(words, reference_words), (index, n_slots)
                # count only
                store.filter_eval_count(code, leaves, n_slots, slot, None)
                assert slot.wait() == int(want.sum()), (index, n_slots)
        finally:
            slot.close()


@pytest.mark.parametrize("n", EVAL_ROWS)
def test_count_slot_evaluator_matches_numpy_and_filter_eval(built, n):
    """A: silo_gpu_filter_eval_count + silo_gpu_count_slot_wait (k_filter_eval_parts<8, 8 | 4, 2>): count, bitset over [0, n), zero
    padding up to row_words * 64, and the words of silo_gpu_filter_eval, with an output bitset and without."""
    _check_count_slot_programs(n)


@pytest.mark.parametrize("n", EVAL_ROWS)
def test_count_slot_evaluator_with_16_leaf_loads_in_flight(built, n):
    """A once more under SILO_GPU_TUNE_EVAL_LEAF_BATCH = 16: the k_filter_eval_parts<16, ...> instantiations."""
    from silo_amd import binding

    lib = binding.load_library()
    previous = lib.silo_gpu_tune(TUNE_EVAL_LEAF_BATCH, 16)
    try:
        _check_count_slot_programs(n)
    finally:
        lib.silo_gpu_tune(TUNE_EVAL_LEAF_BATCH, previous)


@pytest.mark.parametrize("n", [777, 8193, 65_537])
def test_batch_evaluator_slot_classes_in_shuffled_order(built, n):
    """silo_gpu_filter_eval_batch sorts its programs into launches of <= 8, <= 16 and <= 32 slots: the programs of A (1, 2, 4, 6, 12,
    16, 17 and 32 slots, the 19-leaf runs), some without an output bitset.  First a batch of 3, one program of each class with the
    widest first, then one of 40 in a shuffled order, so that the thread's scratch regrows.  Every count equals numpy and
    silo_gpu_filter_eval; every bitset that was asked for equals both, with zero padding."""
    rng = np.random.default_rng(2000 + n)
    masks = _eval_masks(rng, n)
    with _plain_store(n) as store:
        leaves = _upload_masks(store, masks)
        known = _count_slot_programs(masks)
        assert {n_slots for _, n_slots, _ in known} >= {1, 2, 4, 6, 12, 16, 17, 32}
        singles = [_eval(store, code, leaves, n_slots) for code, n_slots, _ in known]  # silo_gpu_filter_eval: (words, count)
        for index, ((words, count), (_, _, want)) in enumerate(zip(singles, known)):
            assert count == int(want.sum()), index
        outs = [store.bitset_alloc() for _ in range(40)]
        by_slots = {n_slots: index for index, (_, n_slots, _) in enumerate(known)}
        for size in (3, 40):
            if size == 3:  # one program of each slot class, the widest first
                order = [by_slots[32], by_slots[1], by_slots[16]]
            else:
                order = [int(i) % len(known) for i in rng.permutation(size)]
                assert set(order) == set(range(len(known)))  # every program, every slot class
            with_bitset = [k % 3 != 1 for k in range(size)]
            for out in outs[:size]:  # all ones: every word the kernel owes is seen
                store.memset(out, 0xFF, store.row_words * 8)
            counts = store.filter_eval_batch([(known[i][0], leaves, known[i][1]) for i in order],
                                             [outs[k] if with_bitset[k] else None for k in range(size)])
            for k, index in enumerate(order):
                want = known[index][2]
                assert counts[k] == int(want.sum()) == singles[index][1], (size, k, index)
                if with_bitset[k]:
                    words = store.bitset_download(outs[k])
                    bits = dense.unpack_bits(words, store.row_words * 64)
                    assert np.array_equal(bits[:n], want), (size, k, index)
                    assert not bits[n:].any(), (size, k, index)
                    assert np.array_equal(words, singles[index][0]), (size, k, index)
        for out in outs:
            store.free(out)


def _reuse_programs(b):
    """(code, n_slots, expected(masks)) — fat (<= 16 slots: 8 waves per block) and thin (> 16: 4 waves, twice the parts) programs
    that select everything, nothing and something.  Seven of them, so that over the launches every program meets both stores
    and every launch differs from the slot's previous launch on the same store."""
    L = b.LEAF_OPERAND
    return [
        (b.encode(b.OP_ONES, 0), 1, lambda m: np.ones(len(m[0]), bool)),
        (b.encode(b.OP_ZERO, 16) + b.encode(b.OP_MOV, 0, 16), 17, lambda m: np.zeros(len(m[0]), bool)),
        (b.encode(b.OP_AND, 0, L + 0, L + 1), 2, lambda m: m[0] & m[1]),
        (b.encode(b.OP_ONES, 31) + b.encode(b.OP_MOV, 0, 31), 32, lambda m: np.ones(len(m[0]), bool)),
        (b.encode(b.OP_ZERO, 0), 1, lambda m: np.zeros(len(m[0]), bool)),
        (b.encode(b.OP_MOV, 16, L + 4) + b.encode(b.OP_NOT, 15, 16) + b.encode(b.OP_OR, 0, 15, L + 1), 17, lambda m: ~m[4] | m[1]),
        (b.encode(b.OP_OR_N, 0, imm=0 | (5 << 16)), 1, lambda m: np.logical_or.reduce(m)),
    ]


def test_one_count_slot_serves_many_launches_of_changing_size(built):
    """ONE slot for 70 consecutive launches that alternate between a 1 200 003-row store (19 or 37 parts) and a 100-row store (one
    part), between fat and thin programs and between filters that select everything and nothing.  What this catches: parts of
    an earlier epoch left in the slot.  After a one-part launch the words 1.. of the slot still hold the parts of the launch
    before it; a wait that counted them, or that took them for this launch's while the kernel is still on its way (each launch
    is queued behind a fill of 64 MB, so the host is at the slot long before the kernel), would report the cardinality of
    another filter.
    (The epoch wraps after 2^32 launches of one slot, where it skips 0; that cannot be reached through the ABI and is not
    simulated here.)"""
    from silo_amd import binding as b

    rng = np.random.default_rng(77)
    sizes = (1_200_003, 100)
    stores = [_plain_store(n) for n in sizes]
    slot = b.CountSlot()
    try:
        masks = [[rng.random(n) < p for p in (0.5, 0.2, 0.7, 0.05, 0.9)] for n in sizes]
        leaves = [_upload_masks(store, m) for store, m in zip(stores, masks)]
        programs = _reuse_programs(b)
        wants = [[int(want(m).sum()) for _, _, want in programs] for m in masks]
        ballast_bytes = 64 << 20
        ballast = stores[0].malloc(ballast_bytes)
        assert len({w for per_store in wants for w in per_store}) >= 8  # the launches do have different answers
        for launch in range(70):
            which = launch % 2
            index = launch % len(programs)
            code, n_slots, _ = programs[index]
            stores[which].memset(ballast, launch & 0xFF, ballast_bytes)  # only enqueued: the evaluator waits behind it
            stores[which].filter_eval_count(code, leaves[which], n_slots, slot)
            assert slot.wait() == wants[which][index], (launch, sizes[which], n_slots)
    finally:
        slot.close()
        for store in stores:
            store.close()


def test_two_count_slots_on_two_streams(built):
    """Launch A, launch B, wait B, wait A: each slot holds its own launch's parts, whichever finishes first."""
    from silo_amd import binding as b

    rng = np.random.default_rng(78)
    n = 1_200_003
    with _plain_store(n) as store:
        masks = [rng.random(n) < p for p in (0.5, 0.2, 0.7, 0.05, 0.9)]
        leaves = _upload_masks(store, masks)
        out_a, out_b = store.bitset_alloc(), store.bitset_alloc()
        store.synchronize()  # the uploads are done before the non-blocking streams start
        streams = [b.GpuStream(), b.GpuStream()]
        slots = [b.CountSlot(), b.CountSlot()]
        try:
            programs = _reuse_programs(b)
            for first, second in ((2, 5), (5, 2), (6, 0), (1, 6), (3, 2)):
                (code_a, slots_a, want_a), (code_b, slots_b, want_b) = programs[first], programs[second]
                store.filter_eval_count(code_a, leaves, slots_a, slots[0], out_a, streams[0].handle)
                store.filter_eval_count(code_b, leaves, slots_b, slots[1], out_b, streams[1].handle)
                count_b = slots[1].wait(streams[1].handle)
                count_a = slots[0].wait(streams[0].handle)
                assert count_a == int(want_a(masks).sum()) and count_b == int(want_b(masks).sum()), (first, second)
                assert np.array_equal(dense.unpack_bits(store.bitset_download(out_a, streams[0].handle), n), want_a(masks))
                assert np.array_equal(dense.unpack_bits(store.bitset_download(out_b, streams[1].handle), n), want_b(masks))
        finally:
            for slot in slots:
                slot.close()
            for stream in streams:
                stream.close()


def test_count_slot_contract(built):
    """A null slot and a program with a bad operand are refused with an error status and launch nothing; the slot that saw the
    refusal answers the next valid launch exactly."""
    from silo_amd import binding as b

    rng = np.random.default_rng(79)
    n = 65_537
    with _plain_store(n) as store:
        masks = [rng.random(n) < p for p in (0.5, 0.2)]
        leaves = _upload_masks(store, masks)
        good = b.encode(b.OP_AND, 0, b.LEAF_OPERAND + 0, b.LEAF_OPERAND + 1)
        want = int((masks[0] & masks[1]).sum())
        slot = b.CountSlot()
        try:
            with pytest.raises(b.SiloGpuError) as refusal:
                store.filter_eval_count(good, leaves, 1, None)
            assert refusal.value.code < 0
            store.filter_eval_count(good, leaves, 1, slot)
            assert slot.wait() == want
            for bad, n_slots in ((b.encode(b.OP_AND, 0, 5, 6), 2),                        # slots 5 and 6 of 2
                                 (b.encode(b.OP_AND, 0, b.LEAF_OPERAND + 2, 0), 1),       # leaf 2 of 2
                                 (b.encode(b.OP_OR_N, 0, imm=1 | (2 << 16)), 1),          # a run past the last leaf
                                 (good, 33)):                                             # more than SILO_GPU_MAX_SLOTS
                with pytest.raises(b.SiloGpuError) as refusal:
                    store.filter_eval_count(bad, leaves, n_slots, slot)
                assert refusal.value.code < 0
                store.filter_eval_count(good, leaves, 1, slot)
                assert slot.wait() == want
                store.filter_eval_count(b.encode(b.OP_ONES, 0), leaves, 1, slot)
                assert slot.wait() == n
        finally:
            slot.close()


# ---- B: the row slot -------------------------------------------------------------------------------------------------------
def _as_set(rows):
    return set(map(tuple, np.asarray(rows).tolist()))


@pytest.mark.parametrize("n_symbols", [5, 22, 32])
@pytest.mark.parametrize("positions", [20000, 1, 255, 256, 257])
def test_row_slot_matches_numpy_and_mutations_select(built, positions, n_symbols):
    """B: silo_gpu_mutations_select_to_slot + silo_gpu_row_slot_wait (k_mutations_select_to_host) on the tables of
    test_mutations_select_threshold_arithmetic_matches_host_doubles, at one block, at the block boundary and at 79 blocks."""
    from silo_amd.binding import RowSlot

    # (a seed per shape; the 20 000-position tables of 5 and 22 symbols are those of the test named above)
    counts, reference, totals = mutations_select_table(n_symbols, positions, None if positions == 20000 else 7 * positions + n_symbols)
    wants = {proportion: mutations_select_expected(counts, reference, totals, proportion) for proportion in MUTATIONS_SELECT_PROPORTIONS}
    sizes = sorted({len(want) for want in wants.values()})
    if positions >= 255:
        assert len(wants[0.0]) > positions and len(sizes) >= 5  # not vacuous
    with make_store(64, [dict(name="s", alphabet="nuc", reference=REFERENCE)]) as store:
        ample = RowSlot(positions * n_symbols)
        try:
            # one slot for the whole list of proportions
            for proportion in MUTATIONS_SELECT_PROPORTIONS:
                want = wants[proportion]
                n, rows = store.mutations_select_to_slot(counts, reference, proportion, ample)
                assert n == len(want) and len(rows) == n, proportion
                assert _as_set(rows) == want, proportion
                n_plain, rows_plain = store.mutations_select(counts, reference, proportion, positions * n_symbols)
                assert n_plain == n and _as_set(rows_plain) == _as_set(rows), proportion
            # slots that are exactly large enough, one row short, and 7 rows long
            for proportion in MUTATIONS_SELECT_PROPORTIONS:
                want = wants[proportion]
                for capacity in sorted({len(want), len(want) - 1, 7} - {0, -1}):
                    slot = RowSlot(capacity)
                    try:
                        n, rows = store.mutations_select_to_slot(counts, reference, proportion, slot)
                        assert n == len(want), (proportion, capacity)  # the true number, whatever fits
                        assert len(rows) == min(n, capacity), (proportion, capacity)
                        delivered = _as_set(rows)
                        assert len(delivered) == len(rows) and delivered <= want, (proportion, capacity)  # pairwise distinct members
                        if n > capacity:
                            # the launch right after an overflowed one, on the same slot, with a list that fits: cursor and ticket
                            # were re-armed inside the kernel
                            fitting = max((p for p in MUTATIONS_SELECT_PROPORTIONS if len(wants[p]) <= capacity), key=lambda p: len(wants[p]), default=None)
                            if fitting is not None:
                                n_next, rows_next = store.mutations_select_to_slot(counts, reference, fitting, slot)
                                assert n_next == len(wants[fitting]) and _as_set(rows_next) == wants[fitting], (proportion, capacity, fitting)
                            n_again, rows_again = store.mutations_select_to_slot(counts, reference, proportion, slot)
                            assert n_again == len(want) and len(rows_again) == capacity and _as_set(rows_again) <= want
                    finally:
                        slot.close()
            # ... and the ample slot after all of that still answers exactly
            n, rows = store.mutations_select_to_slot(counts, reference, 0.05, ample)
            assert n == len(wants[0.05]) and _as_set(rows) == wants[0.05]
        finally:
            ample.close()


def test_row_slot_empty_selection_and_refusals(built):
    """A table of zeros delivers n == 0 (no timeout, no error), also between two launches that select; no positions, no symbols,
    more than 32 symbols and a null slot are refused with an error status, and the slot still serves the next launch."""
    from silo_amd.binding import RowSlot, SiloGpuError

    counts, reference, totals = mutations_select_table(5, 600, 11)
    want = mutations_select_expected(counts, reference, totals, 0.05)
    assert len(want) > 100
    with make_store(64, [dict(name="s", alphabet="nuc", reference=REFERENCE)]) as store:
        slot = RowSlot(600 * 5)
        try:
            for n_positions in (1, 256, 600):
                n, rows = store.mutations_select_to_slot(np.zeros((n_positions, 5), dtype=np.uint32), reference[:n_positions], 0.0, slot)
                assert n == 0 and len(rows) == 0
                n, rows = store.mutations_select_to_slot(counts, reference, 0.05, slot)
                assert n == len(want) and _as_set(rows) == want
            for shape in ((0, 5), (5, 0), (5, 33)):
                with pytest.raises(SiloGpuError) as refusal:
                    store.mutations_select_to_slot(np.zeros(shape, dtype=np.uint32), np.zeros(shape[0], dtype=np.uint8), 0.05, slot)
                assert refusal.value.code < 0, shape
            with pytest.raises(SiloGpuError):
                store.mutations_select_to_slot(counts, reference, 0.05, None)
            n, rows = store.mutations_select_to_slot(counts, reference, 0.05, slot)
            assert n == len(want) and _as_set(rows) == want
        finally:
            slot.close()


# ---- C: dictionary ids -> bitset --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_values", [1, 3, 5000, 70_000])
@pytest.mark.parametrize("n", [1, 64, 777, 300_001])
def test_bitset_from_value_ids_matches_numpy(built, n, n_values):
    """C: silo_gpu_bitset_from_value_ids (k_bitset_from_value_ids) against np.isin and a membership lookup: skewed ids, rows whose
    id is the NULL marker (>= n_values), membership bytes other than 0 and 1, a destination that starts out as all ones."""
    rng = np.random.default_rng(31 * n + n_values)
    ids = rng.integers(0, n_values, size=n).astype(np.uint32)
    ids[rng.random(n) < 0.6] = n_values // 2  # one dominant value
    null = rng.random(n) < 0.02
    ids[null] = rng.choice(np.array([n_values, n_values + 1, 2 * n_values + 5, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint64), size=int(null.sum())).astype(np.uint32)
    if n >= 777:
        ids[1], ids[2] = n_values, 0xFFFFFFFF
        ids[n - 2] = n_values  # in the last, ragged word
    elif n == 1 and n_values == 3:
        ids[0] = n_values
    in_range = ids < n_values
    memberships = [np.zeros(n_values, dtype=np.uint8), np.ones(n_values, dtype=np.uint8),
                   rng.choice(np.array([0, 0, 0, 1, 2, 0x80, 0xFF], dtype=np.uint8), size=n_values)]
    memberships[2][n_values // 2] = 0x80  # the dominant value is a member by a byte that is not 1
    with _plain_store(n) as store:
        ids_dev = store.upload_column(ids)
        out = store.bitset_alloc()
        for membership in memberships:
            want = np.zeros(n, bool)
            want[in_range] = membership[ids[in_range]] != 0
            assert np.array_equal(want, np.isin(ids, np.nonzero(membership)[0]))  # the two references agree
            store.memset(out, 0xFF, store.row_words * 8)
            store.bitset_from_value_ids(out, ids_dev, membership)
            bits = dense.unpack_bits(store.bitset_download(out), store.row_words * 64)
            assert np.array_equal(bits[:n], want)
            assert not bits[n:].any()  # the last ragged word and the padding words
            assert not bits[:n][~in_range].any()
        store.free(ids_dev)


def test_bitset_from_value_ids_refusals(built):
    from silo_amd.binding import SiloGpuError

    n = 777
    with _plain_store(n) as store:
        ids_dev = store.upload_column(np.zeros(n, dtype=np.uint32))
        out = store.bitset_alloc()
        membership = np.ones(3, dtype=np.uint8)
        for arguments in ((out, ids_dev, membership, 0), (out, ids_dev, np.zeros(0, dtype=np.uint8), None), (None, ids_dev, membership, None),
                          (out, None, membership, None), (out, ids_dev, None, 3)):
            with pytest.raises(SiloGpuError) as refusal:
                store.bitset_from_value_ids(*arguments)
            assert refusal.value.code < 0
        store.bitset_from_value_ids(out, ids_dev, membership)
        assert np.array_equal(dense.unpack_bits(store.bitset_download(out), store.row_words * 64), np.arange(store.row_words * 64) < n)
        store.free(ids_dev)


# ---- D: insertion pairs ------------------------------------------------------------------------------------------------------
def _pairs(rng, n, n_pairs, n_ids):
    """(rows, ids) of n_pairs insertion occurrences: several pairs per row, a few hundred pairs inside ONE 64-row word (contended
    atomicOr), one id with about 70 % of the pairs (contended atomicAdd), a pair on the last row."""
    rows = rng.integers(0, n, size=n_pairs).astype(np.uint32)
    repeated = rng.random(n_pairs) < 0.3
    rows[repeated] = rows[rng.integers(0, max(n_pairs, 1), size=int(repeated.sum()))]  # rows with several insertions
    crowd = min(300, n_pairs // 2)
    word = (n // 2) // 64
    crowd_at = rng.choice(n_pairs, size=crowd, replace=False) if crowd else np.zeros(0, dtype=np.int64)
    rows[crowd_at] = np.minimum(word * 64 + rng.integers(0, 64, size=crowd), n - 1)
    ids = rng.integers(0, n_ids, size=n_pairs).astype(np.uint32)
    ids[rng.random(n_pairs) < 0.7] = n_ids // 2
    if n_pairs:
        rows[0] = n - 1
    # the kernels index with these as they are: nothing out of bounds may reach the device
    assert n_pairs == 0 or (int(rows.max()) < n and int(ids.max()) < n_ids)
    return rows, ids


@pytest.mark.parametrize("n_ids", [1, 7, 40_000])
@pytest.mark.parametrize("n_pairs", [0, 1, 255, 256, 257, 500_000])
@pytest.mark.parametrize("n", [100, 300_001])
def test_insertion_pair_kernels_match_numpy(built, n, n_pairs, n_ids):
    """D: silo_gpu_bitset_from_pairs (k_bitset_from_pairs behind its memset) and silo_gpu_count_pairs (k_count_pairs)."""
    from silo_amd.binding import SiloGpuError

    rng = np.random.default_rng(n + 3 * n_pairs + 5 * n_ids)
    rows, ids = _pairs(rng, n, n_pairs, n_ids)
    with _plain_store(n) as store:
        rows_dev = store.upload_column(rows) if n_pairs else None
        ids_dev = store.upload_column(ids) if n_pairs else None
        # K8: dst = rows of the pairs whose id is a member; the destination starts out as all ones
        out = store.bitset_alloc()
        memberships = [np.zeros(n_ids, dtype=np.uint8), np.full(n_ids, 0x40, dtype=np.uint8),
                       rng.choice(np.array([0, 0, 1, 2, 0xFF], dtype=np.uint8), size=n_ids)]
        for membership in memberships:
            want = np.zeros(n, bool)
            want[rows[membership[ids] != 0]] = True
            store.memset(out, 0xFF, store.row_words * 8)
            store.bitset_from_pairs(out, rows_dev, ids_dev, n_pairs, membership)
            bits = dense.unpack_bits(store.bitset_download(out), store.row_words * 64)
            assert np.array_equal(bits[:n], want)
            assert not bits[n:].any()
            if n_pairs and membership[0] == 0x40:
                assert want[n - 1] and bits[n - 1]  # the pair on the last row
        # K9: counts[id] += pairs of the id whose row is in the filter; the table is accumulated into
        nine = np.zeros(n, bool)
        nine[rng.choice(n, size=9, replace=False)] = True
        last = np.zeros(n, bool)
        last[n - 1] = True
        filters = [None, rng.random(n) < 0.4, np.zeros(n, bool), nine, last]
        filter_dev = store.bitset_alloc()
        for mask in filters:
            if mask is None:
                want = np.bincount(ids, minlength=n_ids)
            else:
                want = np.bincount(ids[mask[rows]], minlength=n_ids)
                store.bitset_upload(filter_dev, dense.pack_bits(mask))
            start = rng.integers(1, 1000, size=n_ids).astype(np.uint32)
            counts_dev = store.upload_column(start)
            for _ in range(2):
                store.count_pairs(None if mask is None else filter_dev, rows_dev, ids_dev, n_pairs, counts_dev)
            got = store.read(counts_dev, np.uint32, n_ids)
            assert np.array_equal(got, start + 2 * want.astype(np.uint32))  # n_pairs == 0: untouched
            store.free(counts_dev)
        if n_pairs:
            assert mask is last and want.sum() >= 1  # (the last filter of the list) the pair on row n - 1 was counted
        with pytest.raises(SiloGpuError) as refusal:
            store.count_pairs(None, rows_dev, ids_dev, n_pairs, None)
        assert refusal.value.code < 0
        for pointer in (rows_dev, ids_dev):
            if pointer is not None:
                store.free(pointer)
