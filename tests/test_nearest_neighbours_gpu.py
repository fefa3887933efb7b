"""NearestNeighbours: the rows of the whole database closest to one query sequence (K11), through JSON and the engine: against
distances computed in numpy from the strings the oracle's FastaAligned returns, against DistanceMatrix, and on synthetic stores in
every adaptive layout against numpy on the raw symbol matrix.  Every comparison is an exact equality."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import nearest_rows_reference as ref  # noqa: E402
from tests.pair_distances_reference import AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, PARTITION_SIZES, SEQUENCES, _build_example_engine, _key_is, _tuned_engine  # noqa: E402
from tests.test_distance_matrix_gpu import example, example_data, synthetic  # noqa: E402,F401  (fixtures)
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS  # noqa: E402

FIELDS = {"primaryKey", "distance", "comparedPositions"}
KEY = "gisaid_epi_isl"
_STRINGS = {}  # (sequence, filter) -> [(key, aligned string)] in the order of the data set: the oracle's FastaAligned, asked once each


def _strings(oracle_db, sequence_name, expression):
    name = sequence_name or "main"
    cached = (name, json.dumps(expression, sort_keys=True))
    if cached not in _STRINGS:
        selected = so.execute_query(oracle_db, {"action": {"type": "FastaAligned", "sequenceName": name}, "filterExpression": expression})
        _STRINGS[cached] = [(row[KEY], row[name]) for row in selected]
    return _STRINGS[cached]


def _expected(oracle_db, data, sequence_name, valid_chars, expression, query, k=10, max_distance=None, exclude_key=None):
    """The rows of the response: the selected sequences in the order of the data set (partition, then row), nearest first."""
    order = {key: index for index, key in enumerate(data["keys"])}
    selected = sorted(_strings(oracle_db, sequence_name, expression), key=lambda pair: order[pair[0]])
    if not selected:
        return []
    chars = np.array([list(text.encode()) for _, text in selected], dtype=np.uint8)
    table = ref.query_distances(chars, np.frombuffer(query.encode(), dtype=np.uint8), valid_chars)
    keys = [key for key, _ in selected]
    exclude = keys.index(exclude_key) if exclude_key in keys else None
    return [{"primaryKey": keys[row], "distance": int(table[row, 0]), "comparedPositions": int(table[row, 1])}
            for row in ref.nearest(table, None, k, max_distance, exclude)]


def _action(sequence_name, **fields):
    action = dict(fields, type="NearestNeighbours")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _string_of(oracle_db, sequence_name, key):
    return dict(_strings(oracle_db, sequence_name, {"type": "True"}))[key]


QUERY_ROWS = [0, 37, 40, 99]  # the first row, the only row of the second partition, rows of the third


def test_example_dataset_matches_the_oracles_sequences(example):
    engine, oracle_db, data, _ = example
    filters = [{"type": "True"}, LINEAGE, _key_is(data, 5, 30, 36, 0), _key_is(data, 37), {"type": "False"}]
    for sequence_name, valid_chars in SEQUENCES:
        for row in QUERY_ROWS:
            key = data["keys"][row]
            text = _string_of(oracle_db, sequence_name, key)
            for expression in filters:
                by_key = engine.execute_query({"action": _action(sequence_name, primaryKey=key), "filterExpression": expression})
                assert by_key == _expected(oracle_db, data, sequence_name, valid_chars, expression, text, exclude_key=key), (sequence_name, row, expression)
                by_text = engine.execute_query({"action": _action(sequence_name, sequence=text, neighbours=11), "filterExpression": expression})
                assert by_text == _expected(oracle_db, data, sequence_name, valid_chars, expression, text, k=11), (sequence_name, row, expression)
                assert all(set(entry) == FIELDS for entry in by_key + by_text)
            # the same row's string: the same list plus the row itself at distance 0
            everything = engine.execute_query({"action": _action(sequence_name, primaryKey=key, neighbours=1024), "filterExpression": {"type": "True"}})
            with_self = engine.execute_query({"action": _action(sequence_name, sequence=text, neighbours=1024), "filterExpression": {"type": "True"}})
            assert len(everything) == 99 and len(with_self) == 100
            own = [entry for entry in with_self if entry["primaryKey"] == key]
            assert len(own) == 1 and own[0]["distance"] == 0
            assert [entry for entry in with_self if entry["primaryKey"] != key] == everything
            assert len({entry["distance"] for entry in everything}) > 3 or sequence_name is not None  # not vacuous
            assert all(0 <= entry["distance"] <= entry["comparedPositions"] for entry in everything)


def test_agrees_with_distance_matrix(example):
    """For a selection DistanceMatrix takes, the neighbours of key x are row x of the matrix, sorted."""
    engine, _, data, _ = example
    order = {key: index for index, key in enumerate(data["keys"])}
    for sequence_name, _ in SEQUENCES:
        matrix_action = {"type": "DistanceMatrix"} if sequence_name is None else {"type": "DistanceMatrix", "sequenceName": sequence_name}
        for expression in ({"type": "True"}, LINEAGE):
            pairs = engine.execute_query({"action": matrix_action, "filterExpression": expression})
            assert pairs
            for key in sorted({pair["firstKey"] for pair in pairs})[:3] + [pairs[-1]["secondKey"]]:
                mine = [(pair["distance"], order[pair["secondKey"] if pair["firstKey"] == key else pair["firstKey"]], pair)
                        for pair in pairs if key in (pair["firstKey"], pair["secondKey"])]
                want = [{"primaryKey": pair["secondKey"] if pair["firstKey"] == key else pair["firstKey"], "distance": pair["distance"],
                         "comparedPositions": pair["comparedPositions"]} for _, _, pair in sorted(mine, key=lambda item: item[:2])]
                got = engine.execute_query({"action": _action(sequence_name, primaryKey=key, neighbours=1024), "filterExpression": expression})
                assert got == want, (sequence_name, expression, key)


def test_neighbours_max_distance_order_limit_offset(example):
    engine, oracle_db, data, _ = example
    key = data["keys"][3]
    for sequence_name, valid_chars in SEQUENCES:
        text = _string_of(oracle_db, sequence_name, key)
        full = _expected(oracle_db, data, sequence_name, valid_chars, {"type": "True"}, text, k=1024, exclude_key=key)
        for k in (1, 2, 50, 1024):
            got = engine.execute_query({"action": _action(sequence_name, primaryKey=key, neighbours=k), "filterExpression": {"type": "True"}})
            assert got == full[:k]
        assert engine.execute_query({"action": _action(sequence_name, primaryKey=key), "filterExpression": {"type": "True"}}) == full[:10]  # default
        distances = [entry["distance"] for entry in full]
        for bound in (0, distances[4], distances[4] - 1 if distances[4] else 0, distances[-1]):
            got = engine.execute_query({"action": _action(sequence_name, primaryKey=key, maxDistance=bound, neighbours=20), "filterExpression": {"type": "True"}})
            assert got == [entry for entry in full if entry["distance"] <= bound][:20], (sequence_name, bound)
        base = _action(sequence_name, primaryKey=key, neighbours=30)
        in_python = sorted(full[:30], key=lambda entry: (-entry["comparedPositions"], entry["primaryKey"]))
        ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "comparedPositions", "order": "descending"}, "primaryKey"],
                                                       limit=7, offset=3), "filterExpression": {"type": "True"}})
        assert ordered == in_python[3:10]
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": {"type": "True"}}) == full[2:6]
        assert len(engine.execute_query({"action": dict(base, orderByFields=["distance"], limit=3), "filterExpression": {"type": "True"}})) == 3


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, oracle_db, data, _ = example
    key = data["keys"][0]
    text = _string_of(oracle_db, None, key)
    ok = {"type": "NearestNeighbours", "primaryKey": key}
    cases = [
        ({"type": "NearestNeighbours"}, "primaryKey"),
        (dict(ok, sequence=text), "primaryKey"),
        ({"type": "NearestNeighbours", "sequence": text[:-1]}, "sequence"),
        ({"type": "NearestNeighbours", "sequence": text + "A"}, "sequence"),
        ({"type": "NearestNeighbours", "sequence": 5}, "sequence"),
        ({"type": "NearestNeighbours", "primaryKey": "no such key"}, "no such key"),
        ({"type": "NearestNeighbours", "primaryKey": 1.5}, "primaryKey"),
        ({"type": "NearestNeighbours", "primaryKey": ["a"]}, "primaryKey"),
        ({"type": "NearestNeighbours", "primaryKey": 7}, "primaryKey"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "Database does not contain a sequence with name: 'nosuchsequence'"),
        (dict(ok, neighbours=0), "neighbours"),
        (dict(ok, neighbours=1025), "neighbours"),
        (dict(ok, neighbours="3"), "neighbours"),
        (dict(ok, neighbours=2.5), "neighbours"),
        (dict(ok, maxDistance=-1), "maxDistance"),
        (dict(ok, maxDistance="2"), "maxDistance"),
        (dict(ok, orderByFields=["count"]), "count"),
        (dict(ok, orderByFields=[KEY]), KEY),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (dict(ok, maxDistance=0), dict(ok, neighbours=1024), dict(ok, sequenceName="ORF1a", neighbours=1)):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and all(set(entry) == FIELDS for entry in document["queryResult"]), document


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        action = {"type": "NearestNeighbours", "primaryKey": example_data["keys"][0]}
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"] and "NearestNeighbours" in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions, by key and by a literal sequence, without a filter and under two filters."""
    sym, _, bucket = synthetic
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    chars = lut[sym]
    rows = np.arange(N_ROWS)
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        literal = chars[11].copy()
        literal[::5] = lut[(sym[11, ::5] % 4) + 1]  # a sequence no row has
        literal[7] = ord("?")
        queries = [(dict(primaryKey=str(row)), chars[row], row) for row in (0, 70_000, N_ROWS - 1, int(np.flatnonzero((sym == 15).sum(axis=1) == 5)[0]))]
        queries.append((dict(sequence=bytes(literal).decode()), literal, None))
        for expression, selected in (
            ({"type": "True"}, np.ones(N_ROWS, bool)),
            ({"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7),
            ({"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}, (rows >= 30_000) & (rows <= 61_000)),
        ):
            for fields, query, own_row in queries:
                table = ref.query_distances(chars, query, NUC_VALID)
                for extra in (dict(neighbours=25), dict(neighbours=1024, maxDistance=3)):
                    nearest = ref.nearest(table, selected, extra["neighbours"], extra.get("maxDistance"), own_row)
                    want = [{"primaryKey": str(row), "distance": int(table[row, 0]), "comparedPositions": int(table[row, 1])} for row in nearest]
                    got = engine.execute_query({"action": dict(fields, type="NearestNeighbours", **extra), "filterExpression": expression})
                    assert got == want, (layout, missing_runs, expression, fields if own_row is not None else "literal", extra)
                    assert len(want) == 25 or "maxDistance" in extra  # (a bound may leave nothing of a sequence no row has)
    finally:
        engine.close()
