"""DistinctSequences: the filter expression that keeps one row per distinct aligned sequence of its child's rows (K20), through JSON
and the engine, on the example data set with planted copies as one partition and as three, and on the 140 003 x 48 synthetic stores
in every adaptive layout.  The expected rows come from tests/distinct_reference.py over the data set's row order — the same for
every partitioning.  Every comparison is an exact equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dataset  # noqa: E402
from tests import distinct_reference as ref  # noqa: E402
from tests import sample_reference  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, PARTITION_SIZES, _build_example_engine, _key_is, _tuned_engine  # noqa: E402
from tests.test_distance_matrix_gpu import synthetic  # noqa: E402,F401  (fixture)
from tests.test_distinct_parse import SHARDED, UNKNOWN_SEQUENCE  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS  # noqa: E402
from tests.test_within_distance_gpu import _check_selection, _count_of, _keys_of, _mask_words  # noqa: E402

EVERYTHING = {"type": "True"}
NUC = "-ACGTRYSWKMBDHVN"
AA = "-ACDEFGHIKLMNPQRSTVWYBZ*X"
ORIGINAL, OTHER = 3, 10            # rows that are copied
COPIES = [36, 50, 99]               # of ORIGINAL: in the first and in the third of three partitions
LONE_COPY = 37                      # of OTHER: the only row of the second partition
WITH_N, WITH_CODE = 60, 61          # ORIGINAL with one cell turned into N / into an ambiguity code: rows of their own


def _distinct(child, sequence_name=None):
    expression = {"type": "DistinctSequences", "child": child}
    if sequence_name is not None:
        expression["sequenceName"] = sequence_name
    return expression


@functools.lru_cache(maxsize=None)
def planted_data():
    """The example data set with copies of two rows in the default nucleotide sequence and in the gene S, and two near copies."""
    data = dict(dataset.load_example_dataset())
    data["nuc"] = {name: list(rows) for name, rows in data["nuc"].items()}
    data["aa"] = {name: list(rows) for name, rows in data["aa"].items()}
    for rows, missing, code_for in ((data["nuc"]["main"], "N", {"A": "R", "C": "Y", "G": "R", "T": "Y"}), (data["aa"]["S"], "X", {"D": "B", "N": "B", "E": "Z", "Q": "Z"})):
        assert rows[ORIGINAL] is not None and rows[OTHER] is not None and rows[ORIGINAL] != rows[OTHER]
        for row in COPIES:
            rows[row] = rows[ORIGINAL]
        rows[LONE_COPY] = rows[OTHER]
        text = rows[ORIGINAL]
        at = next(p for p in range(len(text) // 2, len(text)) if text[p] in code_for)
        rows[WITH_N] = text[:at] + missing + text[at + 1:]
        rows[WITH_CODE] = text[:at] + code_for[text[at]] + text[at + 1:]
    return data


@functools.lru_cache(maxsize=None)
def planted_symbols(sequence_name):
    data = planted_data()
    if sequence_name is None:
        return ref.symbols_of_strings(data["nuc"]["main"], NUC, "N", len(data["nuc_references"]["main"]))
    return ref.symbols_of_strings(data["aa"][sequence_name], AA, "X", len(data["aa_references"][sequence_name]))


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def planted(request, built):
    engine = _build_example_engine(planted_data(), request.param)
    yield engine, planted_data(), request.param
    engine.close()


def _mask(engine, data, expression):
    """The rows of the data set an expression without DistinctSequences selects, as the engine answers it."""
    keys = _keys_of(engine, expression)
    return np.array([key in keys for key in data["keys"]])


def _within(data):
    return {"type": "WithinDistance", "primaryKey": data["keys"][ORIGINAL], "maxDistance": 30}


def test_distinct_rows_of_a_child_match_the_reference(planted):
    engine, data, partition_sizes = planted
    n = len(data["keys"])
    sym = planted_symbols(None)
    everything = np.ones(n, dtype=bool)
    want = ref.select(sym, everything)
    # not vacuous: the copies go, the near copies stay, a class has rows in more than one partition
    assert want[ORIGINAL] and want[OTHER] and not want[COPIES].any() and not want[LONE_COPY] and want[WITH_N] and want[WITH_CODE]
    assert 2 < want.sum() <= n - 4
    _check_selection(engine, data, partition_sizes, _distinct(EVERYTHING), want, "True")
    lineage = _mask(engine, data, LINEAGE)
    near = _mask(engine, data, _within(data))
    assert 10 < lineage.sum() < n - 10 and near[ORIGINAL] and near[COPIES].all() and near[WITH_N] and near.sum() > 5
    sampled = sample_reference.select(4, 40, everything)
    late = np.arange(n) > ORIGINAL  # without the original, its first copy represents the class
    for child, selected in ((LINEAGE, lineage), (_within(data), near), ({"type": "Sample", "child": EVERYTHING, "size": 40, "seed": 4}, sampled),
                            ({"type": "Not", "child": _key_is(data, *range(ORIGINAL + 1))}, late), ({"type": "False"}, np.zeros(n, dtype=bool))):
        _check_selection(engine, data, partition_sizes, _distinct(child), ref.select(sym, selected), child["type"])
    assert ref.select(sym, late)[COPIES[0]] and not ref.select(sym, late)[COPIES[1:]].any()
    # a sample of the distinct rows; the distinct rows of the distinct rows
    _check_selection(engine, data, partition_sizes, {"type": "Sample", "child": _distinct(EVERYTHING), "size": 7, "seed": 2},
                     sample_reference.select(2, 7, want), "Sample of DistinctSequences")
    _check_selection(engine, data, partition_sizes, _distinct(_distinct(LINEAGE)), ref.select(sym, lineage), "nested")


def test_a_gene_by_its_name(planted):
    engine, data, partition_sizes = planted
    n = len(data["keys"])
    sym = planted_symbols("S")
    want = ref.select(sym, np.ones(n, dtype=bool))
    assert not want[COPIES].any() and 1 < want.sum() < n and not np.array_equal(want, ref.select(planted_symbols(None), np.ones(n, dtype=bool)))
    _check_selection(engine, data, partition_sizes, _distinct(EVERYTHING, "S"), want, "S")
    _check_selection(engine, data, partition_sizes, _distinct(EVERYTHING, "main"), ref.select(planted_symbols(None), np.ones(n, dtype=bool)), "main")
    lineage = _mask(engine, data, LINEAGE)
    _check_selection(engine, data, partition_sizes, _distinct(LINEAGE, "S"), ref.select(sym, lineage), "S under a lineage")


def test_composition_with_other_expressions(planted):
    engine, data, partition_sizes = planted
    n = len(data["keys"])
    sym = planted_symbols(None)
    lineage = _mask(engine, data, LINEAGE)
    first, second = ref.select(sym, np.ones(n, dtype=bool)), ref.select(planted_symbols("S"), lineage)
    a, b = _distinct(EVERYTHING), _distinct(LINEAGE, "S")
    assert (first & lineage).any() and (first & ~lineage).any() and second.any() and (~first).any()
    cases = [
        ({"type": "And", "children": [a, LINEAGE]}, first & lineage),
        ({"type": "And", "children": [LINEAGE, {"type": "Not", "child": a}]}, lineage & ~first),
        ({"type": "Or", "children": [a, b]}, first | second),
        ({"type": "And", "children": [a, b]}, first & second),
        ({"type": "Not", "child": a}, ~first),
        ({"type": "Not", "child": {"type": "Or", "children": [a, b]}}, ~(first | second)),
        ({"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [a, b, LINEAGE]}, first.astype(int) + second + lineage >= 2),
        ({"type": "N-Of", "numberOfMatchers": 1, "matchExactly": True, "children": [a, b, LINEAGE]}, first.astype(int) + second + lineage == 1),
        ({"type": "Maybe", "child": a}, first),
        ({"type": "Exact", "child": b}, second),
        ({"type": "Not", "child": {"type": "Maybe", "child": b}}, ~second),
        (_distinct({"type": "And", "children": [{"type": "Not", "child": a}, LINEAGE]}), ref.select(sym, ~first & lineage)),
    ]
    for expression, mask in cases:
        _check_selection(engine, data, partition_sizes, expression, mask, expression["type"])


def test_the_child_is_compiled_in_the_mode_of_the_expression(planted):
    engine, data, partition_sizes = planted
    sym = planted_symbols(None)
    position = next(
        (p for p in range(1, 400) if _count_of(engine, {"type": "Maybe", "child": {"type": "NucleotideEquals", "position": p, "symbol": "A"}})
         > _count_of(engine, {"type": "NucleotideEquals", "position": p, "symbol": "A"})), None)
    assert position is not None
    child = {"type": "NucleotideEquals", "position": position, "symbol": "A"}
    exact, maybe = _mask(engine, data, child), _mask(engine, data, {"type": "Maybe", "child": child})
    assert (exact != maybe).any()
    _check_selection(engine, data, partition_sizes, {"type": "Maybe", "child": _distinct(child)}, ref.select(sym, maybe), "maybe")
    _check_selection(engine, data, partition_sizes, _distinct(child), ref.select(sym, exact), "exact")


def test_actions_under_the_expression_equal_those_under_its_keys(planted):
    engine, data, _ = planted
    lineage = _mask(engine, data, LINEAGE)
    rows = np.flatnonzero(ref.select(planted_symbols(None), lineage))
    assert 2 < len(rows) <= lineage.sum()
    actions = [
        {"type": "Mutations", "minProportion": 0.05, "orderByFields": ["mutation"]},
        {"type": "AminoAcidMutations", "sequenceName": "S", "minProportion": 0.05, "orderByFields": ["mutation"]},
        {"type": "DistanceMatrix"},
        {"type": "Aggregated", "groupByFields": ["pango_lineage"], "orderByFields": ["pango_lineage"]},
    ]
    for action in actions:
        got = engine.execute_query({"action": action, "filterExpression": _distinct(LINEAGE)})
        want = engine.execute_query({"action": action, "filterExpression": _key_is(data, *rows)})
        assert got == want and got, action["type"]
    matrix = engine.execute_query({"action": {"type": "DistanceMatrix"}, "filterExpression": _distinct(LINEAGE)})
    assert all(pair["distance"] > 0 or pair["comparedPositions"] < len(data["nuc_references"]["main"]) for pair in matrix)


def test_batch_of_counts_answers_as_single_queries(planted):
    engine, data, _ = planted
    filters = [
        _distinct(EVERYTHING),
        {"type": "And", "children": [LINEAGE, _distinct(EVERYTHING, "S")]},
        _distinct(LINEAGE),
        {"type": "Not", "child": _distinct(_within(data))},
        LINEAGE,
        EVERYTHING,
    ]
    queries = [{"action": {"type": "Aggregated"}, "filterExpression": expression} for expression in filters]
    singles = [engine.execute_query(query) for query in queries]
    batch = engine.execute_batch(queries)
    assert [status for status, _ in batch] == [200] * 6
    assert [document["queryResult"] for _, document in batch] == singles
    n = len(data["keys"])
    assert singles[0][0]["count"] == int(ref.select(planted_symbols(None), np.ones(n, dtype=bool)).sum())
    assert len({single[0]["count"] for single in singles}) > 3


def test_each_error_is_a_bad_request_with_its_message(planted):
    engine, _, _ = planted
    cases = [
        ({"type": "DistinctSequences"}, "The field 'child' is required in a DistinctSequences expression"),
        ({"type": "DistinctSequences", "child": "True"}, "The field 'child' in a DistinctSequences expression needs to be an object"),
        (_distinct(EVERYTHING, 5), "The field 'sequenceName' in a DistinctSequences expression, if present, needs to be a string"),
        (_distinct(EVERYTHING, "nosuchsequence"), UNKNOWN_SEQUENCE.format("nosuchsequence")),
    ]
    for expression, message in cases:
        for wrapped in (expression, {"type": "And", "children": [LINEAGE, {"type": "Not", "child": expression}]}):
            status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": wrapped})
            assert status == 400, (expression, document)
            assert document["error"] == "Bad request" and document["message"] == message, document


@pytest.mark.parametrize("by_position", [False, True], ids=["sequence-shard", "position-shard"])
def test_sharded_engine_refuses(built, by_position):
    engine = _build_example_engine(planted_data(), None)
    try:
        engine.set_sharding(0, 2, by_position)
        status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": _distinct(EVERYTHING)})
        assert status == 400 and document["message"] == SHARDED, document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
_SYNTHETIC_EXPECTED = {}


def synthetic_expected(sym, name, selected):
    """The representatives of the synthetic matrix under a selection (computed once per selection, never changed)."""
    if name not in _SYNTHETIC_EXPECTED:
        want = ref.select(sym, selected)
        want.setflags(write=False)
        _SYNTHETIC_EXPECTED[name] = want
    return _SYNTHETIC_EXPECTED[name]


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):  # noqa: F811
    """140 003 rows x 48 positions: all rows, a scattered selection and a stretch of rows."""
    sym, _, bucket = synthetic
    rows = np.arange(N_ROWS)
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for name, expression, selected in (
            ("all", EVERYTHING, np.ones(N_ROWS, dtype=bool)),
            ("bucket", {"type": "IntBetween", "column": "bucket", "from": 0, "to": 99}, bucket < 100),
            ("stretch", {"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}, (rows >= 30_000) & (rows <= 61_000)),
        ):
            want = synthetic_expected(sym, name, selected)
            assert 1 < want.sum() < selected.sum()  # classes of several rows
            words, count = engine.evaluate_filter(_distinct(expression), partition=0, n_rows=N_ROWS)
            assert np.array_equal(words, _mask_words(want)), (layout, missing_runs, name)
            assert count == int(want.sum()) and _count_of(engine, _distinct(expression)) == count, (layout, missing_runs, name)
        few = engine.execute_query({"action": {"type": "Details", "fields": ["key"]},
                                    "filterExpression": _distinct({"type": "IntBetween", "column": "row", "from": 30_000, "to": 30_400})})
        assert sorted(int(row["key"]) for row in few) == np.flatnonzero(ref.select(sym, (rows >= 30_000) & (rows <= 30_400))).tolist()
    finally:
        engine.close()
