"""tests/roaring_payloads.py (the numpy writer of roaring payloads and the columns of tests/test_roaring_import_shapes_gpu.py)
against oracle/roaring_format.py, and the census of what those columns contain; runs without a GPU."""
import json
import os

import numpy as np
import pytest

from oracle import roaring_format as rf
from tests import roaring_payloads as rp

HERE = os.path.dirname(os.path.abspath(__file__))
VECTORS = json.load(open(os.path.join(HERE, "golden", "roaring", "vectors.json")))["vectors"]


@pytest.mark.parametrize("vector", VECTORS, ids=lambda v: f"{v['name']}-{'runs' if v['use_runs'] else 'plain'}")
def test_serialize_ids_writes_the_committed_vectors(vector):
    payload = bytes.fromhex(vector["payload_hex"])
    ids = rf.deserialize(payload)
    for use_runs in (True, False):
        assert rp.serialize_ids(np.array(ids, dtype=np.int64), use_runs) == rf.serialize(ids, use_runs=use_runs)
    assert rp.serialize_ids(np.array(ids, dtype=np.int64), vector["use_runs"]) == payload
    # any order, duplicates: the same bytes
    shuffled = np.random.default_rng(3).permutation(np.array(ids + ids[:5], dtype=np.int64))
    assert rp.serialize_ids(shuffled, vector["use_runs"]) == payload
    assert rp.container_kinds(payload) == directory_kinds(ids, vector["use_runs"])


def directory_kinds(ids, use_runs):
    """The container kinds of rf.serialize(ids), decided here from the published size rule."""
    kinds = []
    for key in sorted({i >> 16 for i in ids}):
        values = [i for i in ids if i >> 16 == key]
        runs = 1 + sum(1 for a, b in zip(values, values[1:]) if b != a + 1)
        plain = 2 * len(values) if len(values) <= 4096 else 8192
        kinds.append("run" if use_runs and 2 + 4 * runs < plain else ("array" if len(values) <= 4096 else "bitset"))
    return kinds


def test_the_empty_set_and_the_smallest_case():
    for use_runs in (True, False):
        assert rp.serialize_ids(np.zeros(0, dtype=np.int64), use_runs) == rf.serialize([], use_runs=use_runs) == rp.EMPTY
        assert rp.container_kinds(rp.EMPTY) == [] and rp.container_kinds(b"") == []
        case = rp.import_case(rp.SMALLEST)
        for state in rp.STATES:
            for p, (payloads, flipped, deleted) in enumerate(rp.case_payloads(rp.SMALLEST, state, use_runs)):
                column = case.sym[:, p]
                for symbol, payload in payloads.items():
                    ids = np.nonzero(column != symbol if symbol == flipped else column == symbol)[0]
                    assert payload == rf.serialize(ids.tolist(), use_runs=use_runs), (state, p, symbol)
                assert case.missing not in payloads and deleted not in payloads
                assert flipped is None or flipped in payloads
        for row, payload in enumerate(rp.case_missing_rows(rp.SMALLEST, use_runs)):
            assert payload in (b"", rp.EMPTY) or payload == rf.serialize(np.nonzero(case.sym[row] == case.missing)[0].tolist(), use_runs=use_runs)


def test_the_states_of_a_position():
    """position_payloads on a column small enough to read: which symbol is flipped or deleted, and what its payload holds."""
    column = np.array([3, 3, 15, 2, 3, 2, 15, 7], dtype=np.uint8)
    plain, flipped, deleted = rp.position_payloads(column, 16, 15, "plain", True, 2)
    assert (flipped, deleted) == (None, None) and sorted(plain) == [2, 3, 7]
    assert [rf.deserialize(plain[s]) for s in (2, 3, 7)] == [[3, 5], [0, 1, 4], [7]]
    payloads, flipped, deleted = rp.position_payloads(column, 16, 15, "flipped", True, 2)
    assert (flipped, deleted) == (2, None) and rf.deserialize(payloads[2]) == [0, 1, 2, 4, 6, 7] and payloads[3] == plain[3]
    payloads, flipped, deleted = rp.position_payloads(column, 16, 15, "flipped_max", True, 2)
    assert (flipped, deleted) == (3, None) and rf.deserialize(payloads[3]) == [2, 3, 5, 6, 7] and payloads[2] == plain[2]
    payloads, flipped, deleted = rp.position_payloads(column, 16, 15, "deleted", True, 2)
    assert (flipped, deleted) == (None, 3) and sorted(payloads) == [2, 7]
    # a symbol without a row: flipped it is every row, and the payload is there; the lowest id wins among equals
    payloads, flipped, _ = rp.position_payloads(column, 16, 15, "flipped", True, 1)
    assert flipped == 1 and rf.deserialize(payloads[1]) == list(range(8))
    assert rp.position_payloads(np.array([4, 2, 2, 4]), 16, 15, "deleted", True, 1)[2] == 2
    # every row with one symbol: its flipped bitmap is the empty payload, deleted there is no payload at all
    payloads, flipped, _ = rp.position_payloads(np.full(5, 3), 16, 15, "flipped_max", False, 1)
    assert flipped == 3 and payloads == {3: rp.EMPTY}
    assert rp.position_payloads(np.full(5, 3), 16, 15, "deleted", False, 1) == ({}, None, 3)
    # every row missing: no payload, the deleted symbol is the reference symbol
    assert rp.position_payloads(np.full(5, 15), 16, 15, "deleted", True, 4) == ({}, None, 4)
    assert rp.position_payloads(np.full(5, 15), 16, 15, "plain", True, 4) == ({}, None, None)
    rows = rp.missing_row_payloads(np.array([[1, 15, 15, 2], [1, 1, 1, 1], [2, 2, 2, 2], [15, 15, 15, 15]]), 15, True)
    assert rows[1] == rp.EMPTY and rows[2] == b"" and rf.deserialize(rows[0]) == [1, 2] and rf.deserialize(rows[3]) == [0, 1, 2, 3]


def collect(name, use_runs):
    """(kind, cardinality, is_flipped, position, containers of its payload) of every container the GPU test imports for a case."""
    found = []
    for state in rp.STATES:
        for p, (payloads, flipped, _) in enumerate(rp.case_payloads(name, state, use_runs)):
            for symbol, payload in payloads.items():
                directory = rp.container_directory(payload)
                found += [(kind, cardinality, symbol == flipped, p, len(directory)) for kind, cardinality in directory]
    return found


def test_one_payload_of_each_kind_of_the_largest_case_reads_back():
    case = rp.import_case(rp.LARGEST)
    seen = set()
    for use_runs in (True, False):
        for p, (payloads, _, _) in enumerate(rp.case_payloads(rp.LARGEST, "plain", use_runs)):
            for symbol, payload in payloads.items():
                kinds = frozenset(rp.container_kinds(payload))
                if len(kinds) == 1 and not kinds <= seen:
                    seen |= kinds
                    assert rf.deserialize(payload) == np.nonzero(case.sym[:, p] == symbol)[0].tolist(), (p, symbol)
    assert seen == {"array", "bitset", "run"}


def test_census_of_the_generated_cases():
    """What the GPU test relies on meeting; a run there cannot pass by having left a container kind out."""
    with_runs = collect(rp.LARGEST, True)
    for flipped in (True, False):
        assert {kind for kind, _, is_flipped, _, _ in with_runs if is_flipped == flipped} == {"array", "bitset", "run"}, flipped
    without_runs = collect(rp.LARGEST, False)
    assert {kind for kind, *_ in without_runs} == {"array", "bitset"}
    for use_runs, found in ((True, with_runs), (False, without_runs)):
        plain = rp.case_payloads(rp.LARGEST, "plain", use_runs)[4][0]
        assert sorted(plain) == [1, 2, 4]
        assert rp.container_directory(plain[1]) == [("array", 4096)] and rp.container_directory(plain[2]) == [("bitset", 4097)]
        assert sum(1 for kind, cardinality, *_ in found if (kind, cardinality) in (("array", 4096), ("bitset", 4097))) >= 2
        assert any(n_containers == 3 for *_, n_containers in found)
    assert any(rp.container_kinds(payload) == ["run"] for payload in rp.case_missing_rows(rp.LARGEST, True))
    assert not any("run" in rp.container_kinds(payload) for payload in rp.case_missing_rows(rp.LARGEST, False))
    rows = rp.case_missing_rows(rp.LARGEST, True)
    assert b"" in rows and rp.EMPTY in rows


def test_the_columns_are_what_their_description_says():
    for name in rp.case_names() + [rp.EXTRA_PLANE]:
        case = rp.import_case(name)
        n, sym, missing = case.n, case.sym, case.missing
        assert sym.shape == (n, rp.POSITIONS) and sym.max() < case.n_symbols and case.reference.tolist() == rp.REFERENCE.tolist()
        assert np.array_equal(sym, rp._columns(n, case.alphabet, 1000 + n)[0])  # seeded
        assert np.array_equal(sym, rp.import_case(rp.VARIANTS.get(name, name)).sym)
        null = case.is_null.astype(bool)
        assert (sym[null] == missing).all() and np.array_equal(null, (sym == missing).all(axis=1))
        present = sym != missing
        assert (sym[present[:, 3], 3] == 3).all() and not (sym[:, 7] == 1).any() and (sym[:, 1] == missing).sum() <= n // 50
        assert (sym[[r for r in (0, 63, 64, 65535, 65536, n - 1) if r < n and not null[r]], 6] == case.ambiguity).all()
        assert rp.most_numerous_symbol(sym[:, 7], case.n_symbols, missing, 1) != case.reference[7]
        if n <= 64:  # position 5: every row missing — no payloads, a deleted reference symbol without a row
            assert not null.any() and (sym[:, 5] == missing).all()
            assert rp.case_payloads(name, "deleted", True)[5] == ({}, None, 1) and rp.case_payloads(name, "plain", True)[5] == ({}, None, None)
            assert rp.case_payloads(name, "flipped_max", True)[3] == ({3: rp.EMPTY}, 3, None) or (sym[:, 3] == missing).any()
            assert rp.case_payloads(name, "deleted", True)[3] == ({}, None, 3)
        else:
            assert 0 < null.sum() < n // 100 and (sym[:rp.P5_HEAD_ROWS, 5] == missing).all() and (sym[-rp.P5_TAIL_ROWS:, 5] == missing).all()
            assert (sym[:rp.P4_ODD_END, 4] != missing).all()
            assert sym[65536, 2] == 3 or sym[65536, 2] == missing
            # the runs of the missing symbol stay below a quarter of its planes (12 bytes a run): finalize keeps them as runs
            runs = int(((sym == missing) & ~np.c_[np.zeros(n, bool), (sym == missing)[:, :-1]]).sum())
            row_words = (n + 63) // 64
            assert 0 < 12 * runs <= rp.POSITIONS * row_words * 8 // 4
        if case.extra_symbols is not None:
            assert case.extra_symbols == (missing, case.ambiguity) and (sym[:, 6] == case.ambiguity).sum() >= 4
    assert rp.import_case("n1-nuc").sym[0, 3] == 3  # the one row of the smallest store is no null genome
    # the all-missing variant: position 5 of the 65 537-row store as the two small stores have it, every other column unchanged
    base, variant = rp.import_case("n65537-aa"), rp.import_case(rp.ALL_MISSING)
    assert (variant.sym[:, 5] == variant.missing).all() and np.array_equal(np.delete(variant.sym, 5, axis=1), np.delete(base.sym, 5, axis=1))
    assert np.array_equal(variant.is_null, base.is_null) and variant.extra_symbols is None
    assert rp.case_payloads(rp.ALL_MISSING, "deleted", True)[5] == ({}, None, 1)
    payloads, flipped, _ = rp.case_payloads(rp.ALL_MISSING, "flipped", False)[5]
    assert flipped == 1 and rp.container_directory(payloads[1]) == [("bitset", 65536), ("array", 1)]
    assert rp.container_kinds(rp.case_payloads(rp.ALL_MISSING, "flipped", True)[5][0][1]) == ["run", "array"]
