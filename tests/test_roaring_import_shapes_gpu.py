"""silo_gpu_store_import_missing_rows + silo_gpu_store_import_position at the shapes where an import can go wrong: more than one
roaring container, ragged tail words, every container kind under a plain, flipped and deleted symbol, both alphabets, an ambiguity
code as sparse keys and as an extra plane, the identity and the derived layouts — every result compared with numpy on the symbol
matrix the payloads were made from (tests/roaring_payloads.py; its census runs in tests/test_roaring_payloads_reference.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402
from tests import roaring_payloads as rp  # noqa: E402

MATRIX = [(name, state, use_runs) for name in rp.case_names() for state in rp.STATES for use_runs in (True, False)]
MATRIX.append((rp.EXTRA_PLANE, "deleted", True))
MATRIX += [(rp.ALL_MISSING, "deleted", True), (rp.ALL_MISSING, "flipped", False)]
LAYOUT_KNOB, LAUNCH_COST_KNOB = 4, 9


@pytest.mark.parametrize("name,state,use_runs", MATRIX, ids=[f"{name}-{state}-{'runs' if use_runs else 'plain-containers'}" for name, state, use_runs in MATRIX])
def test_imported_store_equals_numpy(built, name, state, use_runs):
    """The store imported from the payloads of a case holds the case's symbol matrix: every one-hot plane, the Mutations scan under
    no filter, a 40 % filter and a filter of the rows at the word and container boundaries, and the reconstructed sequences —
    re-encoded at finalize (knob 0) and with the identity planes kept (knob -1).  A twin store appended from the same characters
    comes out with the same size, plane rows, escape keys and runs: the import left the same build-time planes."""
    from silo_amd import binding

    case = rp.import_case(name)
    n, sym = case.n, case.sym
    positions = rp.POSITIONS
    payloads = rp.case_payloads(name, state, use_runs)
    missing_rows = rp.case_missing_rows(name, use_runs)
    rng = np.random.default_rng(n)
    boundary = case.boundary_rows()
    boundary_mask = np.zeros(n, bool)
    boundary_mask[boundary] = True
    masks = [rng.random(n) < 0.4, boundary_mask]
    picked = np.concatenate([boundary, rng.choice(n, size=min(n, 40), replace=False)]).astype(np.uint32)
    want_planes = {(p, s): dense.pack_bits(sym[:, p] == s) for p in range(positions) for s in range(case.n_symbols)}
    for knob in (0, -1):
        stores = []
        try:
            for twin in (False, True):
                store = binding.GpuStore(n, [case.store_description()])
                stores.append(store)
                store.tune(LAYOUT_KNOB, knob)
                store.tune(LAUNCH_COST_KNOB, -1)
                try:
                    if twin:
                        store.append_sequences(0, 0, case.chars[sym], case.is_null.copy())
                    else:
                        cut = n // 2 + 3 if n >= 8 else n
                        binding.import_missing_rows(store.handle, 0, 0, list(missing_rows[:cut]))
                        if cut < n:
                            binding.import_missing_rows(store.handle, 0, cut, list(missing_rows[cut:]))
                        for p, (bitmaps, flipped, deleted) in enumerate(payloads):
                            binding.import_position(store.handle, 0, p, bitmaps, flipped, deleted)
                    store.finalize()
                finally:
                    store.tune(LAYOUT_KNOB, 0)
                    store.tune(LAUNCH_COST_KNOB, 0)
            store, twin = stores
            scan_symbols = list(store.scan_symbols[0])
            for (p, s), want in want_planes.items():
                got = store.plane_download(0, p, s)
                assert np.array_equal(got[: len(want)], want), (knob, p, s)
                assert not got[len(want):].any(), (knob, p, s)
            assert np.array_equal(store.mutations_scan(0, None), dense.mutation_counts(sym, np.ones(n, bool), scan_symbols)), knob
            for mask in masks:
                ptr = store.bitset_alloc()
                store.bitset_upload(ptr, dense.pack_bits(mask))
                assert np.array_equal(store.mutations_scan(0, ptr), dense.mutation_counts(sym, mask, scan_symbols)), knob
            assert np.array_equal(store.reconstruct_sequences(0, picked), case.chars[sym[picked]]), knob
            identity_rows = positions * (3 if case.alphabet == "nuc" else 5)
            shape = (store.device_bytes, store.scan_rows(0, 0, positions), store.scan_escapes(0), store.scan_runs(0))
            assert shape == (twin.device_bytes, twin.scan_rows(0, 0, positions), twin.scan_escapes(0), twin.scan_runs(0)), knob
            if knob == 0 and n >= 65537 and name in rp.case_names():  # the store really mixes layouts, with derived symbols
                assert shape[1] < identity_rows and shape[3] > 0, shape
            elif knob == 0 and n >= 65537:
                # the two variants keep the plane of the missing symbol, whatever their columns hold — finalize turns only a LONE extra
                # plane into runs, and only where the runs take less than a quarter of it (a column that is missing in every row
                # is a run per row) — and without runs no symbol is derived: scan_runs stays 0.  The amino-acid variant is still
                # re-encoded (one-hot rows and escape keys: by the costs of layout_choice.h about 28 row lengths against 46 for its
                # identity planes); for the 3 identity planes of the nucleotide variant the same sum is too close to call (24.4
                # against 24), there the twin alone says what finalize made of it.
                assert shape[3] == 0 and shape[1] <= identity_rows, shape
                if name == rp.ALL_MISSING:
                    assert shape[1] < identity_rows and shape[2] > 0, shape
            else:
                assert shape[1:] == (identity_rows, 0, 0), (knob, shape)
        finally:
            for store in stores:
                store.close()


LONG_POSITIONS = 65600
LONG_CHECKED = (0, 4095, 4096, 65529, 65530, 65535, 65536, 65544, 65545, 65599)


def long_genome_rows(rng):
    """{row: ids of its missing positions} of a 70-row store with 65 600 positions; every other row has none."""
    scattered = np.sort(rng.choice(65536 // 2, size=5000, replace=False)) * 2  # non-adjacent: no run pays
    scattered = np.concatenate([scattered, [65540, 65550, 65598]])
    past_the_end = np.concatenate([np.arange(100, 200), [300, 65529, 65599, 65600, 70000, 140000, 200000]])
    return {
        0: np.arange(65530, 65545),   # a run over two containers: with runs 2 containers, no offset header
        1: scattered,                 # a bitset container and an array container
        36: np.arange(LONG_POSITIONS),  # a null genome
        37: past_the_end,             # containers 0..3: the offset header, also with runs; the ids past the genome are ignored
        63: scattered + 1,
        64: np.arange(65530, 65545),
        69: np.arange(LONG_POSITIONS),
    }


@pytest.mark.parametrize("use_runs", [True, False], ids=["runs", "plain-containers"])
def test_missing_rows_of_a_long_genome(built, use_runs):
    """The row-wise bitmaps hold POSITIONS: a genome longer than one container, in two calls that split a word of rows.  The plane
    of the missing symbol is read as the import left it (no finalize) at the positions around the container boundaries."""
    from silo_amd import binding

    n = 70
    rows = long_genome_rows(np.random.default_rng(65600))
    payloads = [b"" if row % 2 == 0 else rp.EMPTY for row in range(n)]
    for row, where in rows.items():
        payloads[row] = rp.serialize_ids(where, use_runs)
    payloads[38], payloads[39] = b"", rp.EMPTY
    kinds = {row: rp.container_kinds(payloads[row]) for row in rows}
    if use_runs:
        assert kinds[0] == ["run", "run"] and kinds[36] == ["run", "run"] and kinds[37] == ["run", "array", "array", "array"]
        assert int.from_bytes(payloads[37][:2], "little") == 12347 and int.from_bytes(payloads[0][:2], "little") == 12347
    else:
        assert kinds[0] == ["array", "array"] and kinds[36] == ["bitset", "array"] and kinds[37] == ["array"] * 4
    assert kinds[1] == ["bitset", "array"]
    want = np.zeros((n, LONG_POSITIONS), dtype=bool)
    for row, where in rows.items():
        want[row, where[where < LONG_POSITIONS]] = True
    reference = np.ones(LONG_POSITIONS, dtype=np.uint8)
    with binding.GpuStore(n, [dict(name="s", alphabet="nuc", reference=reference)]) as store:
        binding.import_missing_rows(store.handle, 0, 0, payloads[:37])
        binding.import_missing_rows(store.handle, 0, 37, payloads[37:])
        for p in LONG_CHECKED:
            got = store.read(ctypes.c_void_p(store.plane(0, p, 15)), np.uint64, store.row_words)
            want_plane = dense.pack_bits(want[:, p])
            assert np.array_equal(got[: len(want_plane)], want_plane), p
            assert not got[len(want_plane):].any(), p


REFUSAL_ROWS = 1000
REFUSAL_POSITIONS = 6


def check_the_store_still_works(store, binding, imported=None):
    """After a refused call: a valid import of another position, finalize, and a scan that finds it (and `imported`: {position:
    {symbol: ids}} of what earlier valid calls brought)."""
    n = REFUSAL_ROWS
    evens, odds = np.arange(0, n, 2), np.arange(1, n, 2)
    binding.import_position(store.handle, 0, 5, {1: rp.serialize_ids(evens, True), 4: rp.serialize_ids(odds[:-1], False)})
    store.finalize()
    expected = {5: {1: evens, 4: odds[:-1]}}
    expected.update(imported or {})
    counts = store.mutations_scan(0, None)
    scan_symbols = list(store.scan_symbols[0])
    for position, symbols in expected.items():
        for symbol in range(16):
            want = np.zeros(n, bool)
            want[symbols.get(symbol, np.zeros(0, dtype=np.int64))] = True
            got = store.plane_download(0, position, symbol)
            assert np.array_equal(got[: (n + 63) // 64], dense.pack_bits(want)) and not got[(n + 63) // 64:].any(), (position, symbol)
            if symbol in scan_symbols:
                assert counts[position, scan_symbols.index(symbol)] == want.sum(), (position, symbol)


def refusal_store(binding, extra_plane=False):
    description = dict(name="s", alphabet="nuc", reference=np.ones(REFUSAL_POSITIONS, dtype=np.uint8))
    if extra_plane:
        description["extra_symbols"] = [15, 5]
    return binding.GpuStore(REFUSAL_ROWS, [description])


def ids(*values):
    return rp.serialize_ids(np.array(values, dtype=np.int64), True)


def second_import(store, binding):
    """{A: 3 4 5} and then {R: 4} at the same position: the second call names no scan symbol, so no code bit of the first tells —
    it is refused all the same, and row 4 keeps its one symbol."""
    binding.import_position(store.handle, 0, 0, {1: ids(3, 4, 5)})
    with pytest.raises(binding.SiloGpuError):
        binding.import_position(store.handle, 0, 0, {5: ids(4)})
    with pytest.raises(binding.SiloGpuError):  # rows the first call left alone: still a second import
        binding.import_position(store.handle, 0, 0, {5: ids(700)})
    check_the_store_still_works(store, binding, {0: {1: np.array([3, 4, 5])}})


def overlap_within_one_call(store, binding):
    """One row claimed by a scan symbol and by a sparse symbol within one call."""
    with pytest.raises(binding.SiloGpuError, match="overlap"):
        binding.import_position(store.handle, 0, 1, {1: ids(3, 4, 5), 5: ids(5, 6)})
    check_the_store_still_works(store, binding)


def flipped_without_payload(store, binding):
    """A flipped symbol whose bitmap is not among the payloads is not "no row" but an error; nothing was written, so the same
    position takes the call with the payload there (empty = every row)."""
    with pytest.raises(binding.SiloGpuError):
        binding.import_position(store.handle, 0, 2, {2: ids(7, 8)}, flipped=1)
    with pytest.raises(binding.SiloGpuError):
        binding.import_position(store.handle, 0, 2, {}, flipped=1)
    binding.import_position(store.handle, 0, 2, {1: rp.EMPTY}, flipped=1)
    check_the_store_still_works(store, binding, {2: {1: np.arange(REFUSAL_ROWS)}})


def missing_rows_past_the_end(store, binding):
    last = REFUSAL_ROWS - 1
    with pytest.raises(binding.SiloGpuError):
        binding.import_missing_rows(store.handle, 0, last, [ids(1), ids(2)])
    binding.import_missing_rows(store.handle, 0, last, [ids(1, 2)])
    check_the_store_still_works(store, binding, {1: {15: np.array([last])}, 2: {15: np.array([last])}})


def position_out_of_range(store, binding):
    with pytest.raises(binding.SiloGpuError):
        binding.import_position(store.handle, 0, REFUSAL_POSITIONS, {1: ids(3)})
    check_the_store_still_works(store, binding)


def counting_pass_open(store, binding):
    """Neither call while the counting pass of a two-pass build is open."""
    store.build_pass(0, 1)
    with pytest.raises(binding.SiloGpuError):
        binding.import_position(store.handle, 0, 0, {1: ids(3)})
    with pytest.raises(binding.SiloGpuError):
        binding.import_missing_rows(store.handle, 0, 0, [ids(1)])
    store.build_pass(0, 2)  # (a store of this size keeps its identity planes: the second pass builds them the ordinary way)
    check_the_store_still_works(store, binding)


def after_finalize(store, binding):
    """Neither call after finalize (no further import can follow either): the store answers as before."""
    binding.import_position(store.handle, 0, 0, {2: ids(9, 64)})
    check_the_store_still_works(store, binding, {0: {2: np.array([9, 64])}})
    with pytest.raises(binding.SiloGpuError):
        binding.import_position(store.handle, 0, 1, {1: ids(3)})
    with pytest.raises(binding.SiloGpuError):
        binding.import_missing_rows(store.handle, 0, 0, [ids(1)])
    assert store.mutations_scan(0, None)[0].tolist() == [0, 0, 2, 0, 0]
    assert not store.plane_download(0, 1, 1).any() and not store.plane_download(0, 1, 15).any()


def ids_past_the_end_are_ignored(store, binding):
    """Ids at or past sequence_count inside a payload are no error: ignored, in a plain and in a flipped bitmap."""
    binding.import_position(store.handle, 0, 0, {1: ids(5, 999, 1000, 1001, 1023, 1024, 70000, 140000), 5: ids(6, 1000, 65536 + 6)})
    binding.import_position(store.handle, 0, 1, {2: ids(0, 998, 1000, 66000)}, flipped=2)
    everything_else = np.setdiff1d(np.arange(REFUSAL_ROWS), [0, 998])
    check_the_store_still_works(store, binding, {0: {1: np.array([5, 999]), 5: np.array([6])}, 1: {2: everything_else}})


REFUSALS = [
    ("second-import-sparse-symbol", second_import, False),
    ("second-import-extra-plane-symbol", second_import, True),
    ("overlap-of-scan-and-sparse-symbol", overlap_within_one_call, False),
    ("flipped-without-payload", flipped_without_payload, False),
    ("missing-rows-past-the-end", missing_rows_past_the_end, False),
    ("position-out-of-range", position_out_of_range, False),
    ("counting-pass-open", counting_pass_open, False),
    ("after-finalize", after_finalize, False),
    ("ids-past-the-end-ignored", ids_past_the_end_are_ignored, False),
]


@pytest.mark.parametrize("scenario,extra_plane", [(scenario, extra) for _, scenario, extra in REFUSALS], ids=[name for name, _, _ in REFUSALS])
def test_import_refusals(built, scenario, extra_plane):
    """Every refusal is a SiloGpuError and leaves a store that takes a further import of another position, finalizes and scans."""
    from silo_amd import binding

    with refusal_store(binding, extra_plane) as store:
        scenario(store, binding)
