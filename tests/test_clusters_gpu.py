"""Clusters: the single-linkage clusters of the selected sequences at a distance bound — the connected components of "distance <=
maxDistance and comparedPositions >= minComparedPositions" — from the bit-per-pair kernel and the components kernel (K12), through
JSON and the engine: against the numpy reference of tests/clusters_reference.py on the strings the oracle's FastaAligned returns
for the same filter, against a union-find over the engine's own DistanceMatrix rows, and on synthetic stores in every adaptive
layout against the reference on the raw symbol matrix.  Every comparison is an exact equality."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.clusters_reference import cluster_sizes, components, has_chain, linked_pairs, pair_counts  # noqa: E402
from tests.pair_distances_reference import AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"key", "cluster", "clusterSize"}
# (sequenceName, its valid symbols, a maxDistance at which the example data has structure): the default nucleotide sequence and a gene
SEQUENCES = [(None, NUC_VALID, 8), ("S", AA_VALID, 1)]
NO_BOUND = 0xFFFFFFFF


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


def _rows_of(keys, linked, min_cluster_size=1):
    """(the rows of the response, the labels)."""
    labels = components(linked) if len(keys) else np.zeros(0, np.uint32)
    sizes = cluster_sizes(labels)
    return [{"key": keys[i], "cluster": keys[labels[i]], "clusterSize": int(sizes[i])} for i in range(len(keys)) if sizes[i] >= min_cluster_size], labels


def _action(sequence_name, **fields):
    action = dict(fields, type="Clusters")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data, partition_sizes = example
    filters = [
        ({"type": "True"}, 100),
        (LINEAGE, None),
        (_key_is(data, 40, 3, 99, 57, 38), 5),  # rows of the third partition and one of the first ...
        (_key_is(data, 5, 30, 36, 0), 4),       # ... of the first partition only
        (_key_is(data, 37), 1),                 # one row (the only one of the second partition): one cluster of one
        ({"type": "False"}, 0),
    ]
    partition_of = {key: int(np.searchsorted(np.cumsum(PARTITION_SIZES), row, side="right")) for row, key in enumerate(data["keys"])}
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        for expression, selects in filters:
            keys, differing, compared = _counts(oracle_db, sequence_name, valid_chars, expression)
            linked = linked_pairs(differing, compared, max_distance, 0)
            want, labels = _rows_of(keys, linked)
            if selects == 100:  # the reference itself: the bound finds structure, and single linkage differs from the others here
                sizes = np.bincount(labels)
                assert (sizes > 0).sum() >= 3 and sizes.max() >= 3 and has_chain(linked, labels), (sequence_name, sizes.max())
            got = engine.execute_query({"action": _action(sequence_name, maxDistance=max_distance), "filterExpression": expression})
            assert got == want, (sequence_name, expression)
            assert all(set(row) == FIELDS for row in got)
            if selects is not None:
                assert len(got) == selects
            if selects == 1:
                assert got == [{"key": data["keys"][37], "cluster": data["keys"][37], "clusterSize": 1}]
        if partition_sizes is not None:  # a cluster whose members lie in different partitions
            everything = engine.execute_query({"action": _action(sequence_name, maxDistance=max_distance), "filterExpression": {"type": "True"}})
            assert any(partition_of[row["key"]] != partition_of[row["cluster"]] for row in everything)


def test_agrees_with_a_union_find_over_the_distance_matrix_rows(example):
    engine, _, _, _ = example
    for sequence_name, _, max_distance in SEQUENCES:
        for expression in ({"type": "True"}, LINEAGE):
            matrix_action = {"type": "DistanceMatrix", "maxDistance": max_distance}
            if sequence_name is not None:
                matrix_action["sequenceName"] = sequence_name
            pairs = engine.execute_query({"action": matrix_action, "filterExpression": expression})
            got = engine.execute_query({"action": _action(sequence_name, maxDistance=max_distance), "filterExpression": expression})
            number = {row["key"]: i for i, row in enumerate(got)}
            parent = list(range(len(got)))

            def find(i):
                while parent[i] != i:
                    parent[i] = parent[parent[i]]
                    i = parent[i]
                return i

            for pair in pairs:
                a, b = find(number[pair["firstKey"]]), find(number[pair["secondKey"]])
                parent[max(a, b)] = min(a, b)
            roots = [find(i) for i in range(len(got))]
            assert [row["cluster"] for row in got] == [got[root]["key"] for root in roots]
            assert [row["clusterSize"] for row in got] == [roots.count(root) for root in roots]
            assert len(pairs) > 0 and len(set(roots)) >= 2


def test_min_compared_positions_and_min_cluster_size(example):
    engine, oracle_db, _, _ = example
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        keys, differing, compared = _counts(oracle_db, sequence_name, valid_chars, {"type": "True"})
        near = np.sort(compared[np.triu(differing <= max_distance, 1)])  # the compared positions of the pairs that are linked without it
        without, _ = _rows_of(keys, linked_pairs(differing, compared, max_distance, 0))
        changed = 0
        for min_compared in sorted({int(near[len(near) // 4]) + 1, int(near[len(near) // 2]) + 1, int(near[-1]) + 1}):
            want, _ = _rows_of(keys, linked_pairs(differing, compared, max_distance, min_compared))
            got = engine.execute_query({"action": _action(sequence_name, maxDistance=max_distance, minComparedPositions=min_compared),
                                        "filterExpression": {"type": "True"}})
            assert got == want, (sequence_name, min_compared)
            changed += want != without
        assert changed >= 1 and all(row["clusterSize"] == 1 for row in got)  # (the last bound is above every linked pair's)
        for min_cluster_size in (1, 2, 3, 101):
            want, _ = _rows_of(keys, linked_pairs(differing, compared, max_distance, 0), min_cluster_size)
            got = engine.execute_query({"action": _action(sequence_name, maxDistance=max_distance, minClusterSize=min_cluster_size),
                                        "filterExpression": {"type": "True"}})
            assert got == want and all(row["clusterSize"] >= min_cluster_size for row in got)
        assert got == [] and 0 < len(_rows_of(keys, linked_pairs(differing, compared, max_distance, 0), 3)[0]) < len(keys)


def test_order_limit_offset(example):
    engine, _, _, _ = example
    for sequence_name, _, max_distance in SEQUENCES:
        base = _action(sequence_name, maxDistance=max_distance)
        got = engine.execute_query({"action": base, "filterExpression": {"type": "True"}})
        in_python = sorted(got, key=lambda row: (-row["clusterSize"], row["cluster"], row["key"]))
        assert in_python != got and len({row["clusterSize"] for row in got}) >= 3
        for limit, offset in ((7, 3), (100_000, 0), (5, len(got) - 2)):
            ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "clusterSize", "order": "descending"}, "cluster", "key"],
                                                           limit=limit, offset=offset), "filterExpression": {"type": "True"}})
            assert ordered == in_python[offset:offset + limit]
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": {"type": "True"}}) == got[2:6]


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _, _ = example
    ok = {"type": "Clusters", "maxDistance": 3}
    cases = [
        ({"type": "Clusters"}, "maxDistance"),
        (dict(ok, maxDistance=-1), "maxDistance"),
        (dict(ok, maxDistance=1.5), "maxDistance"),
        (dict(ok, maxDistance="2"), "maxDistance"),
        (dict(ok, maxDistance=None), "maxDistance"),
        (dict(ok, maxDistance=2**31), "maxDistance"),
        (dict(ok, minComparedPositions=-1), "minComparedPositions"),
        (dict(ok, minComparedPositions=0.5), "minComparedPositions"),
        (dict(ok, minComparedPositions="1"), "minComparedPositions"),
        (dict(ok, minComparedPositions=2**31), "minComparedPositions"),
        (dict(ok, minClusterSize=0), "minClusterSize"),
        (dict(ok, minClusterSize=-2), "minClusterSize"),
        (dict(ok, minClusterSize=1.5), "minClusterSize"),
        (dict(ok, minClusterSize="2"), "minClusterSize"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "Database does not contain a sequence with name: 'nosuchsequence'"),
        (dict(ok, orderByFields=["distance"]), "distance"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (dict(ok, maxDistance=0), dict(ok, maxDistance=2**31 - 1, minComparedPositions=2**31 - 1, minClusterSize=1),
                   dict(ok, sequenceName="testSecondSequence"), dict(ok, sequenceName="ORF1a", orderByFields=["key", "cluster", "clusterSize"])):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and document["queryResult"] and all(set(row) == FIELDS for row in document["queryResult"]), document


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        status, document = engine.execute_raw({"action": {"type": "Clusters", "maxDistance": 1}, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"] and "Clusters" in document["message"], document
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
    """(rows, labels, linked) for the rows that `selected` marks; the two counts per pair are computed once per selection."""
    rows = np.flatnonzero(selected)
    if label not in _SYNTHETIC_COUNTS:
        _SYNTHETIC_COUNTS[label] = pair_counts(np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)[sym[rows]], NUC_VALID)
    linked = linked_pairs(*_SYNTHETIC_COUNTS[label], max_distance, min_compared)
    want, labels = _rows_of([str(row) for row in rows], linked)
    return want, labels, linked


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the composition reconstruct -> pack -> within -> components over derived symbols, runs of N,
    sparse ambiguity keys and code planes, for a scattered selection of about 140 rows and a stretch of 401."""
    sym, _, bucket = synthetic
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        rows = np.arange(N_ROWS)
        stretch = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 30_400}
        in_stretch = (rows >= 30_000) & (rows <= 30_400)
        for label, expression, selected in (("bucket", {"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7), ("stretch", stretch, in_stretch)):
            want, labels, linked = _synthetic_expected(sym, selected, label, 0, 46)
            sizes = np.bincount(labels)
            assert (sizes > 0).sum() >= 3 and sizes.max() >= 3 and has_chain(linked, labels)
            got = engine.execute_query({"action": {"type": "Clusters", "maxDistance": 0, "minComparedPositions": 46}, "filterExpression": expression})
            assert got == want, (layout, missing_runs, label)
        # the rows of N glue everything together until the second bound keeps them out
        glued, glued_labels, _ = _synthetic_expected(sym, in_stretch, "stretch", 0, 0)
        apart, apart_labels, _ = _synthetic_expected(sym, in_stretch, "stretch", 0, 40)
        assert len(set(glued_labels.tolist())) == 1 and len(set(apart_labels.tolist())) > 3
        assert engine.execute_query({"action": {"type": "Clusters", "maxDistance": 0}, "filterExpression": stretch}) == glued
        assert engine.execute_query({"action": {"type": "Clusters", "maxDistance": 0, "minComparedPositions": 40}, "filterExpression": stretch}) == apart
    finally:
        engine.close()


def test_the_limit_of_8192_sequences(built, synthetic):
    """Rows 0 .. 8191 — four pack batches, 128 words per row of the matrix — against the reference; rows 0 .. 8192: refused."""
    sym, _, _ = synthetic
    engine = _tuned_engine(synthetic, 0, 0)
    try:
        want, labels, _ = _synthetic_expected(sym, np.arange(N_ROWS) < 8192, "limit", 0, 40)
        assert len(want) == 8192 and len(set(labels.tolist())) >= 3
        got = engine.execute_query({"action": {"type": "Clusters", "maxDistance": 0, "minComparedPositions": 40},
                                    "filterExpression": {"type": "IntBetween", "column": "row", "from": 0, "to": 8191}})
        assert got == want
        status, document = engine.execute_raw({"action": {"type": "Clusters", "maxDistance": 0, "minComparedPositions": 40},
                                               "filterExpression": {"type": "IntBetween", "column": "row", "from": 0, "to": 8192}})
        assert status == 400 and document["message"] == "Clusters action currently limited to 8192 sequences", document
    finally:
        engine.close()
