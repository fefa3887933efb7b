"""MinimumSpanningTree: the minimum spanning forest of the selected sequences over the pairs with "distance <= maxDistance and
comparedPositions >= minComparedPositions", under the strict order of the keys distance * 2^26 + i * 2^13 + j — from the weights
kernel, the one-block forest kernel and the listed-pairs kernel (K13), through JSON and the engine: against the numpy reference of
tests/spanning_reference.py on the strings the oracle's FastaAligned returns for the same filter, against the engine's own Clusters
and DistanceMatrix, and on synthetic stores in every adaptive layout against the reference on the raw symbol matrix.  The forest is
unique, so every comparison is an exact equality."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.clusters_reference import pair_counts  # noqa: E402
from tests.pair_distances_reference import AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402
from tests.spanning_reference import NO_EDGE, cut, forest, key_fields, weights_of  # noqa: E402
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"firstKey", "secondKey", "distance", "comparedPositions"}
# (sequenceName, its valid symbols, a maxDistance at which the example data falls into several trees): the default nucleotide
# sequence and a gene
SEQUENCES = [(None, NUC_VALID, 8), ("S", AA_VALID, 1)]


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data, request.param
    engine.close()


_COUNTS = {}  # (sequence, filter) -> (keys, differing, compared): the oracle's FastaAligned takes seconds per call, so each is asked
#               once — its answer does not depend on how the rows are cut into partitions — and shared, unchanged, by the tests


def _counts(oracle_db, sequence_name, valid_chars, expression):
    name = sequence_name or "main"
    cached = (name, json.dumps(expression, sort_keys=True))
    if cached not in _COUNTS:
        selected = so.execute_query(oracle_db, {"action": {"type": "FastaAligned", "sequenceName": name}, "filterExpression": expression})
        chars = np.array([list(row[name].encode()) for row in selected], dtype=np.uint8).reshape(len(selected), -1) if selected else np.zeros((0, 0), np.uint8)
        _COUNTS[cached] = ([row["gisaid_epi_isl"] for row in selected], *pair_counts(chars, valid_chars))
    return _COUNTS[cached]


def _rows_of(keys, differing, compared, max_distance=NO_EDGE, min_compared=0):
    """(the rows of the response, the keys of the reference forest)."""
    tree = forest(weights_of(differing, compared, max_distance, min_compared)) if len(keys) else np.zeros(0, np.uint64)
    weight, first, second = key_fields(tree)
    rows = [{"firstKey": keys[i], "secondKey": keys[j], "distance": int(w), "comparedPositions": int(compared[i, j])} for w, i, j in zip(weight, first, second)]
    return rows, tree


def _action(sequence_name, **fields):
    action = dict(fields, type="MinimumSpanningTree")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _components(rows, keys):
    """Per key the lowest-numbered key of its tree in the forest `rows`."""
    number = {key: i for i, key in enumerate(keys)}
    parent = list(range(len(keys)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for row in rows:
        a, b = find(number[row["firstKey"]]), find(number[row["secondKey"]])
        parent[max(a, b)] = min(a, b)
    return [keys[find(i)] for i in range(len(keys))]


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data, partition_sizes = example
    filters = [
        ({"type": "True"}, 100),
        (LINEAGE, None),
        (_key_is(data, 40, 3, 99, 57, 38), 5),  # rows of the third partition and one of the first ...
        (_key_is(data, 5, 30, 36, 0), 4),       # ... of the first partition only
        (_key_is(data, 37), 1),                 # one row (the only one of the second partition): no edge
        ({"type": "False"}, 0),
    ]
    partition_of = {key: int(np.searchsorted(np.cumsum(PARTITION_SIZES), row, side="right")) for row, key in enumerate(data["keys"])}
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        for expression, selects in filters:
            keys, differing, compared = _counts(oracle_db, sequence_name, valid_chars, expression)
            for bound in (None, max_distance):
                want, tree = _rows_of(keys, differing, compared, NO_EDGE if bound is None else bound)
                if selects == 100:  # the reference itself: ties among the edges, one tree without a bound and several with it
                    weight = key_fields(tree)[0]
                    assert len(np.unique(weight)) < len(weight) and len(np.unique(weight)) >= 2, sequence_name
                    trees = len(keys) - len(tree)
                    assert (trees == 1) if bound is None else (3 <= trees < len(keys)), (sequence_name, bound, trees)
                fields = {} if bound is None else {"maxDistance": bound}
                got = engine.execute_query({"action": _action(sequence_name, **fields), "filterExpression": expression})
                assert got == want, (sequence_name, expression, bound)
                assert all(set(row) == FIELDS for row in got)
                if selects is not None and selects < 2:
                    assert got == []
                if selects is not None and bound is None:
                    assert len(got) == max(selects - 1, 0)
        if partition_sizes is not None:  # an edge whose ends lie in different partitions
            everything = engine.execute_query({"action": _action(sequence_name), "filterExpression": {"type": "True"}})
            assert any(partition_of[row["firstKey"]] != partition_of[row["secondKey"]] for row in everything)


def test_components_are_the_clusters_of_clusters(example):
    """For several d and c the trees of the bounded forest are the clusters of Clusters with the same fields, and the unbounded
    forest cut at d gives Clusters at d."""
    engine, oracle_db, _, _ = example
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        keys, differing, compared = _counts(oracle_db, sequence_name, valid_chars, {"type": "True"})
        near = np.sort(compared[np.triu(differing <= max_distance, 1)])  # the compared positions of the pairs within the bound
        most = int(compared[np.triu_indices(len(keys), 1)].max())
        unbounded = engine.execute_query({"action": _action(sequence_name), "filterExpression": {"type": "True"}})
        partitions = set()
        for d, c in ((0, 0), (max_distance, 0), (max_distance, int(near[len(near) // 2]) + 1), (3 * max_distance, 0), (2**31 - 1, most + 1)):
            clusters_action = {"type": "Clusters", "maxDistance": d, "minComparedPositions": c}
            if sequence_name is not None:
                clusters_action["sequenceName"] = sequence_name
            clusters = engine.execute_query({"action": clusters_action, "filterExpression": {"type": "True"}})
            assert [row["key"] for row in clusters] == keys
            got = engine.execute_query({"action": _action(sequence_name, maxDistance=d, minComparedPositions=c), "filterExpression": {"type": "True"}})
            assert got == _rows_of(keys, differing, compared, d, c)[0]
            assert _components(got, keys) == [row["cluster"] for row in clusters], (sequence_name, d, c)
            if c == 0:
                assert _components([row for row in unbounded if row["distance"] <= d], keys) == [row["cluster"] for row in clusters]
            partitions.add(len({row["cluster"] for row in clusters}))
        assert len(partitions) >= 3 and len(keys) in partitions  # the bounds change the clusters; the last keeps every sequence alone


def test_every_edge_is_the_distance_matrix_row_of_its_pair(example):
    engine, _, _, _ = example
    for sequence_name, _, max_distance in SEQUENCES:
        for expression in ({"type": "True"}, LINEAGE):
            matrix_action = {"type": "DistanceMatrix"}
            if sequence_name is not None:
                matrix_action["sequenceName"] = sequence_name
            pairs = {(row["firstKey"], row["secondKey"]): row for row in engine.execute_query({"action": matrix_action, "filterExpression": expression})}
            for fields in ({}, {"maxDistance": max_distance}):
                got = engine.execute_query({"action": _action(sequence_name, **fields), "filterExpression": expression})
                assert len(got) > 0 and all(pairs[row["firstKey"], row["secondKey"]] == row for row in got)


def test_order_limit_offset(example):
    engine, _, _, _ = example
    for sequence_name, _, _ in SEQUENCES:
        base = _action(sequence_name)
        got = engine.execute_query({"action": base, "filterExpression": {"type": "True"}})
        assert [row["distance"] for row in got] == sorted(row["distance"] for row in got)  # ascending key order
        in_python = sorted(got, key=lambda row: (-row["distance"], row["secondKey"], row["firstKey"]))
        assert in_python != got and len({row["distance"] for row in got}) >= 3
        for limit, offset in ((7, 3), (100_000, 0), (5, len(got) - 2)):
            ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "distance", "order": "descending"}, "secondKey", "firstKey"],
                                                           limit=limit, offset=offset), "filterExpression": {"type": "True"}})
            assert ordered == in_python[offset:offset + limit]
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": {"type": "True"}}) == got[2:6]


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _, _ = example
    ok = {"type": "MinimumSpanningTree"}
    cases = [
        (dict(ok, maxDistance=-1), "maxDistance"),
        (dict(ok, maxDistance=1.5), "maxDistance"),
        (dict(ok, maxDistance="2"), "maxDistance"),
        (dict(ok, maxDistance=None), "maxDistance"),
        (dict(ok, maxDistance=2**31), "maxDistance"),
        (dict(ok, minComparedPositions=-1), "minComparedPositions"),
        (dict(ok, minComparedPositions=0.5), "minComparedPositions"),
        (dict(ok, minComparedPositions="1"), "minComparedPositions"),
        (dict(ok, minComparedPositions=None), "minComparedPositions"),
        (dict(ok, minComparedPositions=2**31), "minComparedPositions"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "Database does not contain a sequence with name: 'nosuchsequence'"),
        (dict(ok, orderByFields=["cluster"]), "cluster"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (ok, dict(ok, maxDistance=0, minComparedPositions=0), dict(ok, maxDistance=2**31 - 1, minComparedPositions=1),
                   dict(ok, sequenceName="testSecondSequence"),
                   dict(ok, sequenceName="ORF1a", orderByFields=["firstKey", "secondKey", "distance", "comparedPositions"])):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and document["queryResult"] and all(set(row) == FIELDS for row in document["queryResult"]), document
    status, document = engine.execute_raw({"action": dict(ok, minComparedPositions=2**31 - 1), "filterExpression": LINEAGE})
    assert status == 200 and document["queryResult"] == []  # no pair compares at that many positions: no edge, no row


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        status, document = engine.execute_raw({"action": {"type": "MinimumSpanningTree"}, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"] and "MinimumSpanningTree" in document["message"], document
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


_SYNTHETIC_COUNTS = {}


def _synthetic_expected(sym, selected, label, max_distance, min_compared):
    """(rows, keys of the forest) for the rows that `selected` marks; the two counts per pair are computed once per selection."""
    rows = np.flatnonzero(selected)
    if label not in _SYNTHETIC_COUNTS:
        _SYNTHETIC_COUNTS[label] = pair_counts(np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)[sym[rows]], NUC_VALID)
    return _rows_of([str(row) for row in rows], *_SYNTHETIC_COUNTS[label], max_distance, min_compared)


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the composition reconstruct -> pack -> weights -> forest -> listed pairs over derived symbols,
    runs of N, sparse ambiguity keys and code planes, for a scattered selection of about 140 rows and a stretch of 401."""
    sym, _, bucket = synthetic
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        rows = np.arange(N_ROWS)
        stretch = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 30_400}
        in_stretch = (rows >= 30_000) & (rows <= 30_400)
        for label, expression, selected in (("bucket", {"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7), ("stretch", stretch, in_stretch)):
            n = int(selected.sum())
            for fields, bounds in (({}, (NO_EDGE, 0)), ({"minComparedPositions": 40}, (NO_EDGE, 40)), ({"maxDistance": 0, "minComparedPositions": 46}, (0, 46))):
                want, tree = _synthetic_expected(sym, selected, label, *bounds)
                if bounds == (NO_EDGE, 0):
                    assert len(tree) == n - 1  # (in the stretch the rows of N join everything at distance 0)
                if bounds == (NO_EDGE, 40):
                    assert len(np.unique(key_fields(tree)[0])) >= 3 and 2 <= n - len(tree) < n // 4
                if bounds == (0, 46):
                    assert 3 <= n - len(tree) < n  # several trees, not all of one vertex
                got = engine.execute_query({"action": dict(fields, type="MinimumSpanningTree"), "filterExpression": expression})
                assert got == want, (layout, missing_runs, label, bounds)
    finally:
        engine.close()


def test_the_limit_of_8192_sequences(built, synthetic):
    """Rows 0 .. 8191 — four pack batches, a matrix of 256 MB, every vertex slot of the one block — against the reference;
    rows 0 .. 8192: refused."""
    sym, _, _ = synthetic
    engine = _tuned_engine(synthetic, 0, 0)
    try:
        want, tree = _synthetic_expected(sym, np.arange(N_ROWS) < 8192, "limit", NO_EDGE, 40)
        assert len(set(cut(tree, 8192, NO_EDGE).tolist())) >= 2 and len(tree) > 8000
        got = engine.execute_query({"action": {"type": "MinimumSpanningTree", "minComparedPositions": 40},
                                    "filterExpression": {"type": "IntBetween", "column": "row", "from": 0, "to": 8191}})
        assert got == want
        status, document = engine.execute_raw({"action": {"type": "MinimumSpanningTree", "minComparedPositions": 40},
                                               "filterExpression": {"type": "IntBetween", "column": "row", "from": 0, "to": 8192}})
        assert status == 400 and document["message"] == "MinimumSpanningTree action currently limited to 8192 sequences", document
    finally:
        engine.close()
