"""WithinDistance: the filter expression that selects the rows within a distance of one query sequence (K11's table turned into a row
bitset on the device), through JSON and the engine: against distances computed in numpy from the strings the oracle's FastaAligned
returns, composed with the other expressions, under Mutations against the oracle, against NearestNeighbours, and on synthetic stores
in every adaptive layout against numpy on the raw symbol matrix.  Every comparison is an exact equality."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import nearest_rows_reference as ref  # noqa: E402
from tests.pair_distances_reference import NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, SEQUENCES, _build_example_engine, _key_is, _tuned_engine  # noqa: E402
from tests.test_distance_matrix_gpu import example, example_data, synthetic  # noqa: E402,F401  (fixtures)
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS  # noqa: E402
from tests.test_nearest_neighbours_gpu import _string_of, _strings  # noqa: E402

KEY = "gisaid_epi_isl"
QUERY_ROWS = [0, 37, 40, 99]  # the first row, the only row of the second partition, rows of the third
EVERYTHING = {"type": "True"}
_TABLES = {}  # (sequence, query text) -> uint32 [rows of the data set][2] = distance, compared


def _within(sequence_name=None, **fields):
    expression = dict(fields, type="WithinDistance")
    if sequence_name is not None:
        expression["sequenceName"] = sequence_name
    return expression


def _table(oracle_db, data, sequence_name, valid_chars, query_text):
    """(distance, compared) of every row of the data set, in its order, from the oracle's aligned strings."""
    cached = (sequence_name, query_text)
    if cached not in _TABLES:
        strings = dict(_strings(oracle_db, sequence_name, EVERYTHING))
        chars = np.array([list(strings[key].encode()) for key in data["keys"]], dtype=np.uint8)
        _TABLES[cached] = ref.query_distances(chars, np.frombuffer(query_text.encode(), dtype=np.uint8), valid_chars)
    return _TABLES[cached]


def _mask_words(mask):
    padded = np.zeros((len(mask) + 63) // 64 * 64, dtype=bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


def _partition_ranges(n, partition_sizes):
    sizes = partition_sizes or [n]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(starts[k]), int(starts[k + 1])) for k in range(len(sizes))]


def _keys_of(engine, expression):
    rows = engine.execute_query({"action": {"type": "Details", "fields": [KEY]}, "filterExpression": expression})
    keys = [row[KEY] for row in rows]
    assert len(set(keys)) == len(keys)
    return set(keys)


def _count_of(engine, expression):
    return engine.execute_query({"action": {"type": "Aggregated"}, "filterExpression": expression})[0]["count"]


def _check_selection(engine, data, partition_sizes, expression, mask, context):
    """Details, Aggregated and evaluate_filter of every partition against the expected rows of the data set."""
    mask = np.asarray(mask, dtype=bool)
    assert _keys_of(engine, expression) == {data["keys"][row] for row in np.flatnonzero(mask)}, context
    assert _count_of(engine, expression) == int(mask.sum()), context
    for partition, (begin, end) in enumerate(_partition_ranges(len(mask), partition_sizes)):
        words, count = engine.evaluate_filter(expression, partition=partition, n_rows=end - begin)
        assert np.array_equal(words, _mask_words(mask[begin:end])), (context, partition)  # (no bit at or past the partition's rows)
        assert count == int(mask[begin:end].sum()), (context, partition)


def _bounds(table):
    """maxDistance from the reference's sorted distances: the 5th smallest, the median, 0 and the maximum."""
    distances = np.sort(table[:, 0])
    return [int(distances[4]), int(distances[len(distances) // 2]), 0, int(distances[-1])]


def test_example_dataset_matches_the_oracles_sequences(example):
    engine, oracle_db, data, partition_sizes = example
    n = len(data["keys"])
    for sequence_name, valid_chars in SEQUENCES:
        for row in QUERY_ROWS:
            key = data["keys"][row]
            text = _string_of(oracle_db, sequence_name, key)
            table = _table(oracle_db, data, sequence_name, valid_chars, text)
            assert table[row, 0] == 0
            fifth, median, _, largest = _bounds(table)
            if sequence_name is None:  # not vacuous: the bounds cut the data set
                for bound in (fifth, median):
                    assert 2 <= int((table[:, 0] <= bound).sum()) <= n - 1, (row, bound)
            assert int((table[:, 0] <= largest).sum()) == n
            for bound in _bounds(table):
                mask = table[:, 0] <= bound
                assert mask[row]  # a selection contains its own centre
                for fields in (dict(primaryKey=key), dict(sequence=text)):
                    expression = _within(sequence_name, maxDistance=bound, **fields)
                    _check_selection(engine, data, partition_sizes, expression, mask, (sequence_name, row, bound, list(fields)))


def test_composition_with_other_expressions(example):
    engine, oracle_db, data, partition_sizes = example
    keys = data["keys"]
    n = len(keys)
    lineage_keys = {key for key, _ in _strings(oracle_db, None, LINEAGE)}
    lineage = np.array([key in lineage_keys for key in keys])
    assert 0 < lineage.sum() < n
    first_text = _string_of(oracle_db, None, keys[40])
    first_table = _table(oracle_db, data, None, NUC_VALID, first_text)
    first_bound = _bounds(first_table)[1]
    first = first_table[:, 0] <= first_bound
    second_text = _string_of(oracle_db, None, keys[0])
    second_table = _table(oracle_db, data, None, NUC_VALID, second_text)
    second_bound = _bounds(second_table)[0]
    second = second_table[:, 0] <= second_bound
    assert (first != second).any() and (first & lineage).any() and (first & ~lineage).any()
    a = _within(primaryKey=keys[40], maxDistance=first_bound)
    b = _within(sequence=second_text, maxDistance=second_bound)
    votes = first.astype(int) + second.astype(int) + lineage.astype(int)
    cases = [
        ({"type": "And", "children": [a, LINEAGE]}, first & lineage),
        ({"type": "And", "children": [LINEAGE, {"type": "Not", "child": a}]}, lineage & ~first),
        ({"type": "Or", "children": [a, b]}, first | second),
        ({"type": "And", "children": [a, b]}, first & second),
        ({"type": "Not", "child": a}, ~first),
        ({"type": "Not", "child": {"type": "Or", "children": [a, b]}}, ~(first | second)),
        ({"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [a, b, LINEAGE]}, votes >= 2),
        ({"type": "N-Of", "numberOfMatchers": 1, "matchExactly": True, "children": [a, b, LINEAGE]}, votes == 1),
        ({"type": "Maybe", "child": a}, first),
        ({"type": "Exact", "child": a}, first),
        ({"type": "Not", "child": {"type": "Maybe", "child": a}}, ~first),
    ]
    for expression, mask in cases:
        _check_selection(engine, data, partition_sizes, expression, mask, expression["type"])
    assert 0 < (~first).sum() < n  # the complement is within the real rows and not empty


def test_mutations_under_within_distance_match_the_oracle(example):
    engine, oracle_db, data, _ = example
    for sequence_name, valid_chars in SEQUENCES:
        key = data["keys"][0]
        table = _table(oracle_db, data, sequence_name, valid_chars, _string_of(oracle_db, sequence_name, key))
        bound = _bounds(table)[0]
        rows = np.flatnonzero(table[:, 0] <= bound)
        assert len(rows) >= 2
        action = {"type": "Mutations" if sequence_name is None else "AminoAcidMutations", "minProportion": 0.05, "orderByFields": ["mutation"]}
        if sequence_name is not None:
            action["sequenceName"] = sequence_name
        got = engine.execute_query({"action": action, "filterExpression": _within(sequence_name, primaryKey=key, maxDistance=bound)})
        want = so.execute_query(oracle_db, {"action": action, "filterExpression": _key_is(data, *rows)})
        assert got == json.loads(json.dumps(want)) and got, sequence_name


def test_agrees_with_nearest_neighbours(example):
    engine, oracle_db, data, _ = example
    lineage_keys = {key for key, _ in _strings(oracle_db, None, LINEAGE)}
    key = next(key for key in data["keys"] if key in lineage_keys)
    for sequence_name, valid_chars in SEQUENCES:
        text = _string_of(oracle_db, sequence_name, key)
        table = _table(oracle_db, data, sequence_name, valid_chars, text)
        named = {} if sequence_name is None else {"sequenceName": sequence_name}
        for bound in _bounds(table):
            for expression in (LINEAGE, EVERYTHING):
                by_text = engine.execute_query({"action": dict(named, type="NearestNeighbours", sequence=text, neighbours=1024, maxDistance=bound),
                                                "filterExpression": expression})
                within = _keys_of(engine, {"type": "And", "children": [expression, _within(sequence_name, sequence=text, maxDistance=bound)]})
                assert within == {entry["primaryKey"] for entry in by_text}, (sequence_name, bound)
                by_key = engine.execute_query({"action": dict(named, type="NearestNeighbours", primaryKey=key, neighbours=1024, maxDistance=bound),
                                               "filterExpression": expression})
                within = _keys_of(engine, {"type": "And", "children": [expression, _within(sequence_name, primaryKey=key, maxDistance=bound)]})
                assert within == {entry["primaryKey"] for entry in by_key} | {key}, (sequence_name, bound)
                assert key not in {entry["primaryKey"] for entry in by_key}


def test_min_compared_positions(example):
    engine, oracle_db, data, partition_sizes = example
    text = _string_of(oracle_db, None, data["keys"][0])
    position = next(p for p, char in enumerate(text) if char in "ACGT" and p > 300)
    literal = "N" * position + text[position] + "N" * (len(text) - position - 1)
    table = _table(oracle_db, data, None, NUC_VALID, literal)
    assert int(table[:, 1].max()) == 1
    agree = (table[:, 1] == 1) & (table[:, 0] == 0)
    nothing_compared = table[:, 1] == 0
    assert agree.any()
    for minimum, mask in ((0, agree | nothing_compared), (1, agree), (2, np.zeros(len(table), bool))):
        expression = _within(sequence=literal, maxDistance=0, minComparedPositions=minimum)
        _check_selection(engine, data, partition_sizes, expression, mask, minimum)
    everything = _within(sequence=literal, maxDistance=1, minComparedPositions=1)
    _check_selection(engine, data, partition_sizes, everything, table[:, 1] == 1, "compared")


def test_batch_of_counts_answers_as_single_queries(example):
    engine, oracle_db, data, _ = example
    keys = data["keys"]
    text = _string_of(oracle_db, None, keys[37])
    other = _string_of(oracle_db, None, keys[99])
    filters = [
        _within(primaryKey=keys[0], maxDistance=_bounds(_table(oracle_db, data, None, NUC_VALID, _string_of(oracle_db, None, keys[0])))[1]),
        {"type": "And", "children": [LINEAGE, _within(primaryKey=keys[40], maxDistance=30)]},
        _within(sequence=text, maxDistance=_bounds(_table(oracle_db, data, None, NUC_VALID, text))[0]),
        {"type": "Not", "child": _within(sequence=other, maxDistance=12, minComparedPositions=100)},
        LINEAGE,
        EVERYTHING,
    ]
    queries = [{"action": {"type": "Aggregated"}, "filterExpression": expression} for expression in filters]
    singles = [engine.execute_query(query) for query in queries]
    batch = engine.execute_batch(queries)
    assert [status for status, _ in batch] == [200] * 6
    assert [document["queryResult"] for _, document in batch] == singles
    assert len({single[0]["count"] for single in singles}) > 3  # not all the same answer


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, oracle_db, data, _ = example
    key = data["keys"][0]
    text = _string_of(oracle_db, None, key)
    ok = {"type": "WithinDistance", "primaryKey": key, "maxDistance": 3}
    literal = {"type": "WithinDistance", "maxDistance": 3}
    cases = [
        ({"type": "WithinDistance", "maxDistance": 3}, "primaryKey"),
        (dict(ok, sequence=text), "primaryKey"),
        (dict(literal, sequence=text[:-1]), "sequence"),
        (dict(literal, sequence=text + "A"), "sequence"),
        (dict(literal, sequence=5), "sequence"),
        (dict(literal, primaryKey="no such key"), "no such key"),
        (dict(literal, primaryKey=1.5), "primaryKey"),
        (dict(literal, primaryKey=["a"]), "primaryKey"),
        (dict(literal, primaryKey=7), "primaryKey"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "sequenceName"),
        ({"type": "WithinDistance", "primaryKey": key}, "maxDistance"),
        (dict(ok, maxDistance=-1), "maxDistance"),
        (dict(ok, maxDistance="2"), "maxDistance"),
        (dict(ok, maxDistance=2.5), "maxDistance"),
        (dict(ok, maxDistance=2 ** 31), "maxDistance"),
        (dict(ok, minComparedPositions=-1), "minComparedPositions"),
        (dict(ok, minComparedPositions="2"), "minComparedPositions"),
    ]
    for expression, named in cases:
        for wrapped in (expression, {"type": "And", "children": [LINEAGE, {"type": "Not", "child": expression}]}):
            status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": wrapped})
            assert status == 400, (expression, document)
            assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for expression in (dict(ok, maxDistance=0), dict(ok, maxDistance=2 ** 31 - 1, minComparedPositions=0), dict(ok, sequenceName="ORF1a")):
        status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": expression})
        assert status == 200 and document["queryResult"][0]["count"] >= 1, document


@pytest.mark.parametrize("by_position", [False, True], ids=["sequence-shard", "position-shard"])
def test_sharded_engine_refuses(built, example_data, by_position):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, by_position)
        for fields in (dict(primaryKey=example_data["keys"][0]), dict(sequence="A")):
            status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": _within(maxDistance=2, **fields)})
            assert status == 400 and "sharded" in document["message"] and "WithinDistance" in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions, by key and by a literal sequence, alone and under two filters."""
    sym, _, bucket = synthetic
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    chars = lut[sym]
    rows = np.arange(N_ROWS)
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        literal = chars[11].copy()
        literal[::5] = lut[(sym[11, ::5] % 4) + 1]  # a sequence no row has
        literal[7] = ord("?")
        assert not (chars == literal[None, :]).all(axis=1).any()
        queries = [(dict(primaryKey=str(row)), chars[row], row) for row in (0, 70_000, N_ROWS - 1)]
        queries.append((dict(sequence=bytes(literal).decode()), literal, None))
        for fields, query, own_row in queries:
            table = ref.query_distances(chars, query, NUC_VALID)
            for bound in (0, 3, POSITIONS):
                near = table[:, 0] <= bound
                if own_row is not None:
                    assert near[own_row]
                    if bound == 3:
                        assert 1 < int(near.sum()) < N_ROWS  # not vacuous
                if bound == POSITIONS:
                    assert near.all()
                for expression, selected in (
                    (EVERYTHING, np.ones(N_ROWS, bool)),
                    ({"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7),
                    ({"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}, (rows >= 30_000) & (rows <= 61_000)),
                ):
                    both = {"type": "And", "children": [expression, _within(maxDistance=bound, **fields)]}
                    context = (layout, missing_runs, expression, fields if own_row is not None else "literal", bound)
                    assert _count_of(engine, both) == int((near & selected).sum()), context
                    words, count = engine.evaluate_filter(both)
                    assert np.array_equal(words, _mask_words(near & selected)), context
                    assert count == int((near & selected).sum()), context
        # minComparedPositions keeps the rows without anything to compare (whole genomes missing) out of a neighbourhood
        table = ref.query_distances(chars, chars[0], NUC_VALID)
        assert (table[:, 1] == 0).any()
        expression = _within(primaryKey="0", maxDistance=3, minComparedPositions=1)
        words, count = engine.evaluate_filter(expression)
        assert np.array_equal(words, _mask_words((table[:, 0] <= 3) & (table[:, 1] >= 1))) and count < _count_of(engine, _within(primaryKey="0", maxDistance=3))
    finally:
        engine.close()
