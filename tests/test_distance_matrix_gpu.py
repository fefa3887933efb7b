"""DistanceMatrix: per unordered pair of the selected sequences the positions where both hold a valid mutation symbol and where those
differ, from the pair kernel (K10), through JSON and the engine: against distances computed in numpy from the strings the oracle's
FastaAligned returns for the same filter, and on synthetic stores in every adaptive layout against numpy on the raw symbol
matrix.  Every comparison is an exact equality."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.pair_distances_reference import AA_VALID, NUC_CHARS, NUC_VALID, pair_distances  # noqa: E402
from tests.test_mutations_over_time_gpu import (  # noqa: E402
    N_ROWS, _build_example_engine, _synthetic_dates, _synthetic_engine, _synthetic_matrix)
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"firstKey", "secondKey", "distance", "comparedPositions"}
PARTITION_SIZES = [37, 1, 62]
SEQUENCES = [(None, NUC_VALID), ("S", AA_VALID)]  # the default nucleotide sequence (main) and a gene


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data, request.param
    engine.close()


def _rows_of(keys, table):
    n = len(keys)
    return [{"firstKey": keys[i], "secondKey": keys[j], "distance": int(table[i, j, 0]), "comparedPositions": int(table[i, j, 1])}
            for i in range(n) for j in range(i + 1, n)]


_EXPECTED = {}  # (sequence, filter) -> the rows: the oracle's FastaAligned takes seconds per call, so each is asked once — its answer
#                 does not depend on how the rows are cut into partitions (partition order, then row id = the order of the data set)


def _expected(oracle_db, sequence_name, valid_chars, expression):
    """Every row of the response from the strings of the oracle's FastaAligned for the same filter."""
    name = sequence_name or "main"
    cached = (name, json.dumps(expression, sort_keys=True))
    if cached not in _EXPECTED:
        selected = so.execute_query(oracle_db, {"action": {"type": "FastaAligned", "sequenceName": name}, "filterExpression": expression})
        chars = np.array([list(row[name].encode()) for row in selected], dtype=np.uint8).reshape(len(selected), -1) if selected else np.zeros((0, 0), np.uint8)
        _EXPECTED[cached] = _rows_of([row["gisaid_epi_isl"] for row in selected], pair_distances(chars, valid_chars))
    return _EXPECTED[cached]


def _action(sequence_name, **fields):
    action = dict(fields, type="DistanceMatrix")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _key_is(data, *rows):
    children = [{"type": "StringEquals", "column": "gisaid_epi_isl", "value": data["keys"][row]} for row in rows]
    return children[0] if len(children) == 1 else {"type": "Or", "children": children}


def test_example_dataset_matches_the_oracles_sequences(example):
    engine, oracle_db, data, partition_sizes = example
    filters = [
        ({"type": "True"}, 100),
        (LINEAGE, None),
        (_key_is(data, 40, 3, 99, 57, 38), 5),  # rows of the third partition and one of the first ...
        (_key_is(data, 5, 30, 36, 0), 4),       # ... of the first partition only
        (_key_is(data, 37), 1),                 # one row (the only one of the second partition): no pair
        ({"type": "False"}, 0),
    ]
    partition_of = {key: int(np.searchsorted(np.cumsum(PARTITION_SIZES), row, side="right")) for row, key in enumerate(data["keys"])}
    for sequence_name, valid_chars in SEQUENCES:
        for expression, selects in filters:
            got = engine.execute_query({"action": _action(sequence_name), "filterExpression": expression})
            want = _expected(oracle_db, sequence_name, valid_chars, expression)
            assert got == want, (sequence_name, expression)
            assert all(set(row) == FIELDS for row in got)
            if selects is not None:
                assert len(got) == selects * (selects - 1) // 2
            if expression in (filters[0][0], filters[1][0]):  # not vacuous
                assert len(got) > 20 and len({row["distance"] for row in got}) > 3
                assert all(0 <= row["distance"] <= row["comparedPositions"] for row in got)
        if partition_sizes is not None:  # pairs whose rows lie in different partitions, and in the same one
            everything = engine.execute_query({"action": _action(sequence_name), "filterExpression": {"type": "True"}})
            across = [row for row in everything if partition_of[row["firstKey"]] != partition_of[row["secondKey"]]]
            assert across and len(across) < len(everything)
            assert {(partition_of[row["firstKey"]], partition_of[row["secondKey"]]) for row in across} == {(0, 1), (0, 2), (1, 2)}
            assert any(row["comparedPositions"] > 0 for row in across)


def test_max_distance(example):
    engine, oracle_db, _, _ = example
    for sequence_name, valid_chars in SEQUENCES:
        for expression in ({"type": "True"}, LINEAGE):
            everything = _expected(oracle_db, sequence_name, valid_chars, expression)
            distances = sorted(row["distance"] for row in everything)
            middle = distances[len(distances) // 2]
            if middle == distances[-1]:  # (more than half the pairs at the greatest distance: take the one below)
                middle = max(d for d in distances if d < middle)
            assert distances[0] <= middle < distances[-1]  # some pairs pass, not all
            for max_distance in (0, middle):
                got = engine.execute_query({"action": _action(sequence_name, maxDistance=max_distance), "filterExpression": expression})
                assert got == [row for row in everything if row["distance"] <= max_distance], (sequence_name, expression, max_distance)
            assert 0 < len(got) < len(everything)


def test_order_limit_offset(example):
    engine, _, _, _ = example
    for sequence_name, _ in SEQUENCES:
        base = _action(sequence_name)
        got = engine.execute_query({"action": base, "filterExpression": LINEAGE})
        in_python = sorted(got, key=lambda row: (-row["distance"], row["firstKey"], row["secondKey"]))
        assert in_python != got and len({row["distance"] for row in in_python}) > 10
        for limit, offset in ((7, 3), (100_000, 0), (5, len(got) - 2)):
            ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "distance", "order": "descending"}, "firstKey", "secondKey"],
                                                           limit=limit, offset=offset), "filterExpression": LINEAGE})
            assert ordered == in_python[offset:offset + limit]
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": LINEAGE}) == got[2:6]
        assert len(engine.execute_query({"action": dict(base, orderByFields=["comparedPositions"], limit=3), "filterExpression": LINEAGE})) == 3


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _, _ = example
    ok = {"type": "DistanceMatrix"}
    cases = [
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "Database does not contain a sequence with name: 'nosuchsequence'"),
        (dict(ok, maxDistance=-1), "maxDistance"),
        (dict(ok, maxDistance=1.5), "maxDistance"),
        (dict(ok, maxDistance="2"), "maxDistance"),
        (dict(ok, maxDistance=None), "maxDistance"),
        (dict(ok, orderByFields=["count"]), "count"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (dict(ok, maxDistance=0), dict(ok, sequenceName="testSecondSequence"), dict(ok, sequenceName="ORF1a", maxDistance=100_000)):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and all(set(row) == FIELDS for row in document["queryResult"]), document


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        status, document = engine.execute_raw({"action": {"type": "DistanceMatrix"}, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"] and "DistanceMatrix" in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2026)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


def _tuned_engine(synthetic, layout, missing_runs):
    from silo_amd import binding

    lib = binding.load_library()
    lib.silo_gpu_tune(4, layout)
    lib.silo_gpu_tune(9, -1)
    lib.silo_gpu_tune(8, missing_runs)
    try:
        return _synthetic_engine(*synthetic)[0]
    finally:
        lib.silo_gpu_tune(4, 0)
        lib.silo_gpu_tune(9, 0)
        lib.silo_gpu_tune(8, 0)


def _synthetic_expected(sym, selected):
    rows = np.flatnonzero(selected)
    chars = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)[sym[rows]]
    return [str(row) for row in rows], pair_distances(chars, NUC_VALID)


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the composition reconstruct -> pack -> pairs over derived symbols, runs of N, sparse ambiguity
    keys and code planes, for a scattered selection of about 140 rows and a stretch of 401."""
    sym, _, bucket = synthetic
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        rows = np.arange(N_ROWS)
        for expression, selected in (
            ({"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7),
            ({"type": "IntBetween", "column": "row", "from": 30_000, "to": 30_400}, (rows >= 30_000) & (rows <= 30_400)),
        ):
            keys, table = _synthetic_expected(sym, selected)
            assert 100 < len(keys) < 500
            got = engine.execute_query({"action": {"type": "DistanceMatrix"}, "filterExpression": expression})
            assert got == _rows_of(keys, table), (layout, missing_runs, expression)
            upper = table[np.triu_indices(len(keys), 1)]
            assert (upper[:, 0] > 0).any() and (upper[:, 1] < 48).any()
    finally:
        engine.close()


def test_the_limit_of_2048_sequences(built, synthetic):
    """Rows 0 .. 2047: 2 048 x 2 047 / 2 pairs, of which only the number at distance 0 is compared (maxDistance 0) and the last
    three are looked at (offset); rows 0 .. 2048: refused."""
    sym, _, _ = synthetic
    engine = _tuned_engine(synthetic, 0, 0)
    try:
        at_limit = {"type": "IntBetween", "column": "row", "from": 0, "to": 2047}
        keys, table = _synthetic_expected(sym, np.arange(N_ROWS) < 2048)
        pairs = 2048 * 2047 // 2
        upper = table[np.triu_indices(2048, 1)]
        assert len(upper) == pairs
        at_zero = int((upper[:, 0] == 0).sum())
        assert 0 < at_zero < pairs
        status, body = engine.execute_text({"action": {"type": "DistanceMatrix", "maxDistance": 0}, "filterExpression": at_limit})
        assert status == 200 and body.count(b'"distance":0,') == body.count(b'"distance":') == at_zero
        got = engine.execute_query({"action": {"type": "DistanceMatrix", "offset": pairs - 3, "limit": 10}, "filterExpression": at_limit})
        assert got == _rows_of(keys[-3:], table[-3:, -3:])  # the last three of all pairs
        status, document = engine.execute_raw({"action": {"type": "DistanceMatrix", "maxDistance": 0},
                                               "filterExpression": {"type": "IntBetween", "column": "row", "from": 0, "to": 2048}})
        assert status == 400 and document["message"] == "DistanceMatrix action currently limited to 2048 sequences", document
    finally:
        engine.close()
