"""DistinctSequenceCounts: the action that lists the largest classes of equal aligned sequences of a selection with their sizes
(K21), through JSON and the engine, on the example data set with planted copies (tests/test_distinct_gpu.py) as one partition and as
three, and on the 140 003 x 48 synthetic stores in every adaptive layout.  The expected rows come from
tests/distinct_counts_reference.py over the data set's row order — the same for every partitioning.  Every comparison is an exact
equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import distinct_counts_reference as counts_ref  # noqa: E402
from tests import sample_reference  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, PARTITION_SIZES, _build_example_engine, _tuned_engine  # noqa: E402
from tests.test_distance_matrix_gpu import synthetic  # noqa: E402,F401  (fixture)
from tests.test_distinct_gpu import COPIES, EVERYTHING, LONE_COPY, ORIGINAL, OTHER, _distinct, _mask, _within, planted_data, planted_symbols  # noqa: E402
from tests.test_distinct_sequence_counts_parse import SHARDED, UNKNOWN_SEQUENCE  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS  # noqa: E402
from tests.test_within_distance_gpu import _count_of, _keys_of  # noqa: E402

DEFAULT_CLASSES = 1024


def _action(**fields):
    return dict(fields, type="DistinctSequenceCounts")


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def planted(request, built):
    engine = _build_example_engine(planted_data(), request.param)
    yield engine, planted_data()
    engine.close()


def _rows(data, keys):
    """The response rows of an array of class keys, in its order."""
    return [{"count": count, "primaryKey": data["keys"][row]} for count, row in counts_ref.unpack(keys)]


def _expected(data, sym, selected, min_count=1, max_classes=DEFAULT_CLASSES):
    return _rows(data, counts_ref.first_keys(counts_ref.classes(sym, selected), max_classes, min_count))


def _answer(engine, expression, **fields):
    return engine.execute_query({"action": _action(**fields), "filterExpression": expression})


def test_the_classes_of_a_selection_match_the_reference(planted):
    engine, data = planted
    n = len(data["keys"])
    sym = planted_symbols(None)
    everything = np.ones(n, dtype=bool)
    got = _answer(engine, EVERYTHING)
    assert got == _expected(data, sym, everything)
    # not vacuous: the planted copies make the two largest classes, and the rest follows
    assert got[0] == {"count": 4, "primaryKey": data["keys"][ORIGINAL]} and got[1] == {"count": 2, "primaryKey": data["keys"][OTHER]}
    assert len(COPIES) == 3 and LONE_COPY != OTHER and len(got) > 10
    # the counts sum to the filter's cardinality; the keys are the rows DistinctSequences keeps
    assert sum(row["count"] for row in got) == _count_of(engine, EVERYTHING) == n
    assert {row["primaryKey"] for row in got} == _keys_of(engine, _distinct(EVERYTHING))
    lineage = _mask(engine, data, LINEAGE)
    near = _mask(engine, data, _within(data))
    sampled = sample_reference.select(4, 40, everything)
    for child, selected in ((LINEAGE, lineage), (_within(data), near), ({"type": "Sample", "child": EVERYTHING, "size": 40, "seed": 4}, sampled),
                            ({"type": "False"}, np.zeros(n, dtype=bool))):
        got = _answer(engine, child)
        assert got == _expected(data, sym, selected), child["type"]
        assert sum(row["count"] for row in got) == _count_of(engine, child) == int(selected.sum()), child["type"]
        assert {row["primaryKey"] for row in got} == _keys_of(engine, _distinct(child)), child["type"]
    assert _answer(engine, {"type": "False"}) == []
    assert near[ORIGINAL] and near[COPIES].all() and _answer(engine, _within(data))[0]["count"] == 4


def test_a_gene_by_its_name(planted):
    engine, data = planted
    n = len(data["keys"])
    everything = np.ones(n, dtype=bool)
    got = _answer(engine, EVERYTHING, sequenceName="S")
    assert got == _expected(data, planted_symbols("S"), everything) and got != _answer(engine, EVERYTHING)
    assert got[0]["count"] >= 4 and sum(row["count"] for row in got) == n
    assert {row["primaryKey"] for row in got} == _keys_of(engine, _distinct(EVERYTHING, "S"))
    assert _answer(engine, EVERYTHING, sequenceName="main") == _expected(data, planted_symbols(None), everything)
    lineage = _mask(engine, data, LINEAGE)
    assert _answer(engine, LINEAGE, sequenceName="S") == _expected(data, planted_symbols("S"), lineage)


def test_min_count_and_max_classes(planted):
    engine, data = planted
    n = len(data["keys"])
    sym = planted_symbols(None)
    everything = np.ones(n, dtype=bool)
    for max_classes in (1, 2, 16384):
        got = _answer(engine, EVERYTHING, maxClasses=max_classes)
        assert got == _expected(data, sym, everything, max_classes=max_classes), max_classes
    assert len(_answer(engine, EVERYTHING, maxClasses=1)) == 1 and len(_answer(engine, EVERYTHING, maxClasses=2)) == 2
    got = _answer(engine, EVERYTHING, minCount=2)
    assert got == _expected(data, sym, everything, min_count=2) and [row["count"] for row in got] == [4, 2]
    assert _answer(engine, EVERYTHING, minCount=2, maxClasses=1) == _expected(data, sym, everything, min_count=2, max_classes=1)
    assert _answer(engine, EVERYTHING, minCount=4) == _expected(data, sym, everything, min_count=4) != []
    assert _answer(engine, EVERYTHING, minCount=5) == []
    assert _answer(engine, EVERYTHING, minCount=2 ** 31 - 1) == []


def test_order_limit_offset(planted):
    engine, data = planted
    n = len(data["keys"])
    rows = _expected(data, planted_symbols(None), np.ones(n, dtype=bool))
    for descending in (False, True):
        order = "descending" if descending else "ascending"
        got = _answer(engine, EVERYTHING, orderByFields=[{"field": "primaryKey", "order": order}])
        assert got == sorted(rows, key=lambda row: row["primaryKey"], reverse=descending), order
        got = _answer(engine, EVERYTHING, orderByFields=[{"field": "count", "order": order}, "primaryKey"])
        assert got == sorted(sorted(rows, key=lambda row: row["primaryKey"]), key=lambda row: row["count"], reverse=descending), order
        got = _answer(engine, EVERYTHING, orderByFields=[{"field": "count", "order": order}])  # (rows of equal counts in any order)
        assert [row["count"] for row in got] == sorted((row["count"] for row in rows), reverse=descending), order
        assert sorted(got, key=lambda row: row["primaryKey"]) == sorted(rows, key=lambda row: row["primaryKey"]), order
    assert _answer(engine, EVERYTHING, limit=3) == rows[:3]
    assert _answer(engine, EVERYTHING, limit=3, offset=1) == rows[1:4]
    assert _answer(engine, EVERYTHING, offset=len(rows) - 2) == rows[-2:]
    assert _answer(engine, EVERYTHING, offset=len(rows) + 5) == []
    # maxClasses cuts before the ordering, limit after it
    by_key = _answer(engine, EVERYTHING, maxClasses=5, orderByFields=["primaryKey"], limit=2)
    assert by_key == sorted(rows[:5], key=lambda row: row["primaryKey"])[:2]


def test_batch_answers_as_single_queries(planted):
    engine, _ = planted
    queries = [
        {"action": _action(), "filterExpression": EVERYTHING},
        {"action": _action(minCount=2, sequenceName="S"), "filterExpression": LINEAGE},
        {"action": {"type": "Aggregated"}, "filterExpression": _distinct(EVERYTHING)},
    ]
    singles = [engine.execute_query(query) for query in queries]
    batch = engine.execute_batch(queries)
    assert [status for status, _ in batch] == [200] * 3
    assert [document["queryResult"] for _, document in batch] == singles
    assert singles[0][0]["count"] == 4 and singles[2][0]["count"] == len(singles[0])


def test_each_error_is_a_bad_request_with_its_message(planted):
    engine, _ = planted
    cases = [
        (_action(sequenceName="nosuchsequence"), UNKNOWN_SEQUENCE.format("nosuchsequence")),
        (_action(orderByFields=["distance"]), "OrderByField distance is not contained in the result of this operation."),
        (_action(minCount=0), "DistinctSequenceCounts action: the field minCount, if present, must be an integer of at least 1"),
        (_action(maxClasses=16385), "DistinctSequenceCounts action: the field maxClasses, if present, must be an integer from 1 to 16384"),
    ]
    for action, message in cases:
        for expression in (EVERYTHING, LINEAGE):
            status, document = engine.execute_raw({"action": action, "filterExpression": expression})
            assert status == 400, (action, document)
            assert document["error"] == "Bad request" and document["message"] == message, document


@pytest.mark.parametrize("by_position", [False, True], ids=["sequence-shard", "position-shard"])
def test_sharded_engine_refuses(built, by_position):
    engine = _build_example_engine(planted_data(), None)
    try:
        engine.set_sharding(0, 2, by_position)
        status, document = engine.execute_raw({"action": _action(), "filterExpression": EVERYTHING})
        assert status == 400 and document["message"] == SHARDED, document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
_SYNTHETIC_EXPECTED = {}


def synthetic_expected(sym, name, selected):
    """[(count, row)] of the 16 384 largest classes of the synthetic matrix under a selection (computed once per selection)."""
    if name not in _SYNTHETIC_EXPECTED:
        classes = counts_ref.classes(sym, selected)
        _SYNTHETIC_EXPECTED[name] = (tuple(counts_ref.unpack(counts_ref.first_keys(classes, 16384))), len(classes))
    return _SYNTHETIC_EXPECTED[name]


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):  # noqa: F811
    """140 003 rows x 48 positions: all rows (more classes than an answer lists), a scattered selection and a stretch of rows."""
    sym, _, bucket = synthetic
    rows = np.arange(N_ROWS)
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for name, expression, selected in (
            ("all", EVERYTHING, np.ones(N_ROWS, dtype=bool)),
            ("bucket", {"type": "IntBetween", "column": "bucket", "from": 0, "to": 99}, bucket < 100),
            ("stretch", {"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}, (rows >= 30_000) & (rows <= 61_000)),
        ):
            want, n_classes = synthetic_expected(sym, name, selected)
            assert want[0][0] > 1 and 1 < n_classes < selected.sum()  # classes of several rows
            got = _answer(engine, expression, maxClasses=16384)
            assert [(row["count"], int(row["primaryKey"])) for row in got] == list(want), (layout, missing_runs, name)
            if n_classes <= 16384:
                assert sum(row["count"] for row in got) == int(selected.sum()), name
        assert synthetic_expected(sym, "all", None)[1] > 16384  # the selection on the device had something to leave out
        few = _answer(engine, EVERYTHING, minCount=synthetic_expected(sym, "all", None)[0][5][0], maxClasses=16384)
        assert [(row["count"], int(row["primaryKey"])) for row in few] == [pair for pair in synthetic_expected(sym, "all", None)[0]
                                                                           if pair[0] >= synthetic_expected(sym, "all", None)[0][5][0]]
    finally:
        engine.close()
