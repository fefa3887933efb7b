"""Consensus / AminoAcidConsensus: the consensus sequence of the rows a filter selects, or of each of up to 64 named groups under it,
from the exact Mutations scan and the consensus call (K15), through JSON and the engine: against the numpy reference of
tests/consensus_reference.py applied to the strings the oracle's FastaAligned returns for the same filter, against the engine's own
single requests and its Mutations rows, and on synthetic stores in every adaptive layout against the reference on the raw symbol
matrix.  Every comparison is an exact equality.

The counts that the tests assert of the reference before they compare (main = the default nucleotide sequence, 29 903 positions; S =
the gene, 1 274; the lineage is B.1.1.7 with its sublineages, 51 of the 100 rows) were worked out on the CPU with the oracle.  At
threshold 0.5 main / all rows has 3 ambiguous positions: at 1 the shortest prefix already holds two symbols, at 2 a symbol tied with
the last one of the prefix comes along (a tie at the cut)."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.consensus_reference import VALID, consensus_row, count_table  # noqa: E402
from tests.pair_distances_reference import NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"name", "sequenceName", "count", "consensus", "ambiguousPositions", "lowCoveragePositions", "deletedPositions", "differences"}
ORDERABLE = ["name", "count", "ambiguousPositions", "lowCoveragePositions", "deletedPositions", "differences"]
SEQUENCES = [(None, "main", "nuc"), ("S", "S", "aa")]  # (sequenceName of the request, the store, its alphabet)
THRESHOLDS = (0.5, 0.75, 0.9, 1.0)
TRUE = {"type": "True"}
FALSE = {"type": "False"}


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


_CHARS = {}  # (store, filter) -> (keys, chars): the oracle's FastaAligned takes seconds per call, so each is asked once — its answer
#              does not depend on how the rows are cut into partitions — and shared, unchanged, by the tests


def _chars(oracle_db, store, expression):
    cached = (store, json.dumps(expression, sort_keys=True))
    if cached not in _CHARS:
        selected = so.execute_query(oracle_db, {"action": {"type": "FastaAligned", "sequenceName": store}, "filterExpression": expression})
        chars = np.array([list(row[store].encode()) for row in selected], dtype=np.uint8).reshape(len(selected), -1) if selected else np.zeros((0, 0), np.uint8)
        _CHARS[cached] = ([row["gisaid_epi_isl"] for row in selected], chars)
    return _CHARS[cached]


def _reference_of(data, store, alphabet):
    return (data["nuc_references"] if alphabet == "nuc" else data["aa_references"])[store]


def _both(oracle_db, store, *expressions):
    """The characters of the rows that every one of the expressions selects, in the order of the data set."""
    keys, chars = _chars(oracle_db, store, TRUE)
    wanted = [set(_chars(oracle_db, store, expression)[0]) for expression in expressions]
    rows = [row for row, key in enumerate(keys) if all(key in selected for selected in wanted)]
    return chars[rows]


def _want(data, oracle_db, store, alphabet, expressions, threshold=0.5, min_depth=1, name=None):
    reference = _reference_of(data, store, alphabet)
    return dict(consensus_row(_both(oracle_db, store, *expressions), reference, alphabet, threshold, min_depth), name=name, sequenceName=store)


def _action(sequence_name, alphabet, **fields):
    action = dict(fields, type="Consensus" if alphabet == "nuc" else "AminoAcidConsensus")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _cut(chars, alphabet, threshold):
    """(depth, positions where the shortest prefix holds several symbols, positions where a symbol tied with the prefix's last comes
    along, positions whose call holds '-' and something else) of the reference's table: what the pre-checked counts are about."""
    table = count_table(chars, alphabet).astype(np.int64)
    depth = table.sum(axis=1)
    descending = -np.sort(-table, axis=1)
    last = (np.cumsum(descending, axis=1) >= np.ceil(depth * threshold)[:, None]).argmax(axis=1)
    taken = (table >= descending[np.arange(len(last)), last][:, None]) & (depth[:, None] > 0)
    return depth, int(((last > 0) & (depth > 0)).sum()), int((taken.sum(axis=1) > last + 1).sum()), int((taken[:, 0] & (taken.sum(axis=1) > 1)).sum())


def _filters(data):
    """all rows, the lineage, keys spanning partitions, one row, no row"""
    return [TRUE, LINEAGE, _key_is(data, 40, 3, 99, 57, 38), _key_is(data, 37), FALSE]


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        positions = len(_reference_of(data, store, alphabet))
        for expression in _filters(data):
            chars = _both(oracle_db, store, expression)
            for threshold in THRESHOLDS:
                want = _want(data, oracle_db, store, alphabet, [expression], threshold)
                if expression in (TRUE, LINEAGE):  # the reference itself, case by case
                    depth, several, ties, with_gap = _cut(chars, alphabet, threshold)
                    case = (store, expression == TRUE, threshold)
                    if store == "main" and expression == TRUE:
                        assert (int(depth.min()), int(depth.max())) == (45, 100)
                        assert {0.5: (3, 1, 2), 0.75: (62, 62, 0), 0.9: (169, 169, 0)}.get(threshold, (want["ambiguousPositions"], several, ties)) == (want["ambiguousPositions"], several, ties), case
                        assert threshold != 0.75 or with_gap == 38
                    if store == "main" and expression == LINEAGE:
                        assert len(chars) == 51 and (int(depth.min()), int(depth.max())) == (19, 51)
                        assert threshold != 0.75 or want["ambiguousPositions"] == 27
                    if store == "S" and expression == LINEAGE:
                        assert threshold != 0.75 or ties >= 1
                    if store == "S" and expression == TRUE:
                        assert (int(depth.min()), int(depth.max())) == (88, 100)
                    assert want["differences"] > 0 or threshold == 1.0
                got = engine.execute_query({"action": _action(sequence_name, alphabet, threshold=threshold), "filterExpression": expression})
                assert got == [want], (store, expression, threshold)
                assert set(got[0]) == FIELDS and len(got[0]["consensus"]) == positions and got[0]["count"] == len(chars)
            if expression == FALSE:  # a group that selects nothing still gets a row
                assert got[0]["count"] == 0 and got[0]["consensus"] == ("N" if alphabet == "nuc" else "X") * positions and got[0]["lowCoveragePositions"] == positions
            if expression == _key_is(data, 37):  # one row: its own valid symbols, the missing symbol elsewhere, at every threshold
                assert got[0]["ambiguousPositions"] == 0 and got[0]["count"] == 1
        default = engine.execute_query({"action": _action(sequence_name, alphabet), "filterExpression": LINEAGE})
        assert default == [_want(data, oracle_db, store, alphabet, [LINEAGE], 0.5, 1)]  # threshold 0.5 and minDepth 1 are the defaults


def test_min_depth_from_the_references_depths(example):
    engine, oracle_db, data = example
    cases = [(None, "main", "nuc", TRUE, 60, 72), (None, "main", "nuc", LINEAGE, 20, 1), ("S", "S", "aa", TRUE, 89, None), ("S", "S", "aa", TRUE, 101, 1274)]
    for sequence_name, store, alphabet, expression, min_depth, low in cases:
        for threshold in (0.5, 0.9):
            want = _want(data, oracle_db, store, alphabet, [expression], threshold, min_depth)
            assert want["lowCoveragePositions"] == low if low is not None else want["lowCoveragePositions"] >= 1
            got = engine.execute_query({"action": _action(sequence_name, alphabet, threshold=threshold, minDepth=min_depth), "filterExpression": expression})
            assert got == [want], (store, expression, min_depth, threshold)
            missing = "N" if alphabet == "nuc" else "X"
            assert got[0]["consensus"].count(missing) >= got[0]["lowCoveragePositions"]


def _nine_groups(data):
    """More than one scan batch; `none` selects nothing, `lineage` and `again` select the same rows, `spanning` and `overlap` share rows."""
    return [("all", TRUE), ("lineage", LINEAGE), ("spanning", _key_is(data, 40, 3, 99, 57, 38)), ("one", _key_is(data, 37)), ("none", FALSE),
            ("again", {"type": "And", "children": [LINEAGE, TRUE]}), ("others", {"type": "Not", "child": LINEAGE}),
            ("overlap", _key_is(data, 40, 3, 12, 60, 37)), ("first", _key_is(data, 5, 30, 36, 0))]


def test_nine_groups_are_nine_single_requests(example):
    engine, oracle_db, data = example
    groups = _nine_groups(data)
    as_json = [{"name": name, "filterExpression": expression} for name, expression in groups]
    for sequence_name, store, alphabet in SEQUENCES:
        for query_filter in (TRUE, LINEAGE):  # a group ANDs with the query's filter
            for threshold, min_depth in ((0.5, 1), (0.75, 2)):
                got = engine.execute_query({"action": _action(sequence_name, alphabet, groups=as_json, threshold=threshold, minDepth=min_depth), "filterExpression": query_filter})
                assert [row["name"] for row in got] == [name for name, _ in groups]  # in the order of `groups`
                for row, (name, expression) in zip(got, groups):
                    both = {"type": "And", "children": [query_filter, expression]}
                    single = engine.execute_query({"action": _action(sequence_name, alphabet, threshold=threshold, minDepth=min_depth), "filterExpression": both})
                    assert single[0]["name"] is None and dict(single[0], name=name) == row, (store, name, threshold)
                    assert row == _want(data, oracle_db, store, alphabet, [query_filter, expression], threshold, min_depth, name), (store, name, threshold)
                by_name = {row["name"]: row for row in got}
                assert by_name["none"]["count"] == 0 and dict(by_name["again"], name="lineage") == by_name["lineage"]
                assert by_name["others"]["count"] == (49 if query_filter == TRUE else 0) and by_name["lineage"]["count"] == 51
                assert by_name["spanning"]["count"] == (5 if query_filter == TRUE else len(_both(oracle_db, store, LINEAGE, groups[2][1])))
        one_group = engine.execute_query({"action": _action(sequence_name, alphabet, groups=as_json[1:2]), "filterExpression": TRUE})
        assert one_group == [_want(data, oracle_db, store, alphabet, [LINEAGE], name="lineage")]


def test_every_covered_difference_is_a_mutations_row_at_or_above_the_threshold(example):
    engine, _, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        reference = _reference_of(data, store, alphabet)
        mutations_type = "Mutations" if alphabet == "nuc" else "AminoAcidMutations"
        for expression in (TRUE, LINEAGE):
            rows = engine.execute_query({"action": {"type": mutations_type, "sequenceName": store, "minProportion": 0}, "filterExpression": expression})
            proportion = {row["mutation"]: row["proportion"] for row in rows}
            for threshold in THRESHOLDS:
                got = engine.execute_query({"action": _action(sequence_name, alphabet, threshold=threshold), "filterExpression": expression})[0]
                differing = [p for p, call in enumerate(got["consensus"]) if call in VALID[alphabet] and call != reference[p]]
                assert len(differing) == got["differences"] and (differing or store == "S")
                for p in differing:
                    mutation = f"{reference[p]}{p + 1}{got['consensus'][p]}"
                    assert proportion.get(mutation, -1.0) >= threshold, (store, expression, threshold, mutation)
                assert got["consensus"].count("-") == got["deletedPositions"]


def test_order_limit_offset(example):
    engine, _, data = example
    as_json = [{"name": name, "filterExpression": expression} for name, expression in _nine_groups(data)]
    for sequence_name, _, alphabet in SEQUENCES:
        base = _action(sequence_name, alphabet, groups=as_json, threshold=0.9)
        got = engine.execute_query({"action": base, "filterExpression": TRUE})
        assert len(got) == 9
        for field in ORDERABLE:
            for descending in (False, True):
                order_by = [{"field": field, "order": "descending" if descending else "ascending"}, "name"]
                want = sorted(sorted(got, key=lambda row: row["name"]), key=lambda row: row[field], reverse=descending)  # (stable: ties stay by name)
                for limit, offset in ((4, 2), (100, 0), (3, 7)):
                    ordered = engine.execute_query({"action": dict(base, orderByFields=order_by, limit=limit, offset=offset), "filterExpression": TRUE})
                    assert ordered == want[offset:offset + limit], (field, descending)
            assert len({row[field] for row in got}) >= (3 if field in ("name", "count") else 2) or alphabet == "aa"  # something to put in order
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": TRUE}) == got[2:6]
        assert engine.execute_query({"action": dict(base, offset=9), "filterExpression": TRUE}) == []


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _ = example
    ok = {"type": "Consensus"}
    group = {"name": "a", "filterExpression": TRUE}
    cases = [
        (dict(ok, threshold=0), "threshold"),
        (dict(ok, threshold=-0.5), "threshold"),
        (dict(ok, threshold=1.5), "threshold"),
        (dict(ok, threshold="0.5"), "threshold"),
        (dict(ok, threshold=None), "threshold"),
        (dict(ok, threshold=[0.5]), "threshold"),
        (dict(ok, minDepth=0), "minDepth"),
        (dict(ok, minDepth=-1), "minDepth"),
        (dict(ok, minDepth=1.5), "minDepth"),
        (dict(ok, minDepth="1"), "minDepth"),
        (dict(ok, minDepth=None), "minDepth"),
        (dict(ok, minDepth=2**32), "minDepth"),
        (dict(ok, groups=group), "groups"),
        (dict(ok, groups="a"), "groups"),
        (dict(ok, groups=None), "groups"),
        (dict(ok, groups=[]), "groups"),
        (dict(ok, groups=[TRUE, 5]), "groups"),
        (dict(ok, groups=[{"filterExpression": TRUE}]), "name"),
        (dict(ok, groups=[{"name": 5, "filterExpression": TRUE}]), "name"),
        (dict(ok, groups=[group, dict(group)]), "'a' occurs more than once"),
        (dict(ok, groups=[{"name": "a"}]), "filterExpression of the group 'a'"),
        (dict(ok, groups=[{"name": "a", "filterExpression": "True"}]), "filterExpression of the group 'a'"),
        (dict(ok, groups=[group, {"name": "b", "filterExpression": {"type": "NoSuchFilter"}}]), "filterExpression of the group 'b'"),
        (dict(ok, groups=[group, {"name": "b", "filterExpression": {"column": "pango_lineage"}}]), "filterExpression of the group 'b'"),
        (dict(ok, groups=[{"name": "c", "filterExpression": {"type": "FloatBetween", "column": "nosuchcolumn", "from": 0.5, "to": 1.5}}]), "filterExpression of the group 'c'"),
        (dict(ok, groups=[{"name": "c", "filterExpression": {"type": "FloatBetween", "column": "nosuchcolumn", "from": 0.5, "to": 1.5}}]), "nosuchcolumn"),
        (dict(ok, groups=[{"name": str(g), "filterExpression": TRUE} for g in range(65)]), "limit of 64"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "'nosuchsequence'"),
        (dict(ok, sequenceName="S"), "'S'"),  # a gene is no nucleotide sequence
        ({"type": "AminoAcidConsensus"}, "sequenceName"),
        ({"type": "AminoAcidConsensus", "sequenceName": "main"}, "'main'"),
        (dict(ok, orderByFields=["consensus"]), "consensus"),
        (dict(ok, orderByFields=["sequenceName"]), "sequenceName"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (ok, dict(ok, threshold=1, minDepth=2**32 - 1), dict(ok, threshold=1e-9, minDepth=1, groups=[group]),
                   dict(ok, sequenceName="testSecondSequence"), dict(ok, groups=[{"name": str(g), "filterExpression": TRUE} for g in range(64)], orderByFields=ORDERABLE),
                   {"type": "AminoAcidConsensus", "sequenceName": "ORF1a", "orderByFields": ORDERABLE}):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and document["queryResult"] and all(set(row) == FIELDS for row in document["queryResult"]), document
        assert len(document["queryResult"]) == len(action.get("groups", [0]))


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        for action in ({"type": "Consensus"}, {"type": "AminoAcidConsensus", "sequenceName": "S"}):
            status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
            assert status == 400 and "sharded" in document["message"] and action["type"] in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2027)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the exact scan over derived symbols, runs of N, sparse ambiguity keys and code planes, then the
    call, for the whole store (the cached totals), a lineage-like range of rows, and 8 + 1 groups (a second scan batch) under each."""
    sym, _, bucket = synthetic
    reference = "".join(NUC_VALID[1 + (p % 4)] for p in range(POSITIONS))  # as _synthetic_engine gives it
    chars = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)[sym]
    rows = np.arange(N_ROWS)
    in_range = (rows >= 30_000) & (rows <= 61_000)
    stretch = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}
    groups = [(f"bucket{b}", {"type": "IntBetween", "column": "bucket", "from": 100 * b, "to": 100 * b + 99 - 10 * b}, (bucket >= 100 * b) & (bucket <= 100 * b + 99 - 10 * b))
              for b in range(8)] + [("early", {"type": "IntBetween", "column": "row", "from": 0, "to": 45_000}, rows <= 45_000)]
    as_json = [{"name": name, "filterExpression": expression} for name, expression, _ in groups]
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for query_filter, mask in ((TRUE, np.ones(N_ROWS, dtype=bool)), (stretch, in_range)):
            median_depth = int(np.sort(count_table(chars[mask], "nuc").sum(axis=1))[POSITIONS // 2])  # as minDepth: about half the positions are low
            for threshold, min_depth in ((0.5, 1), (0.9, 2), (1.0, median_depth)):
                want = dict(consensus_row(chars[mask], reference, "nuc", threshold, min_depth), name=None, sequenceName="main")
                got = engine.execute_query({"action": {"type": "Consensus", "threshold": threshold, "minDepth": min_depth}, "filterExpression": query_filter})
                assert got == [want], (layout, missing_runs, query_filter, threshold)
                if threshold == 1.0:  # not vacuous: ambiguous and low-coverage positions, deletions and differences all occur
                    assert 0 < want["ambiguousPositions"] and 0 < want["lowCoveragePositions"] < POSITIONS
                else:
                    assert want["deletedPositions"] > 0 and want["differences"] > want["deletedPositions"]
            for threshold, min_depth in ((0.75, 1), (0.9, 3000)):
                want = [dict(consensus_row(chars[mask & group], reference, "nuc", threshold, min_depth), name=name, sequenceName="main") for name, _, group in groups]
                got = engine.execute_query({"action": {"type": "Consensus", "groups": as_json, "threshold": threshold, "minDepth": min_depth}, "filterExpression": query_filter})
                assert got == want, (layout, missing_runs, query_filter, threshold)
                assert all(row["count"] > 0 for row in got)
                if min_depth == 3000 and query_filter == stretch:  # not vacuous: groups below the depth everywhere, and groups above it
                    assert 0 < sum(row["lowCoveragePositions"] == POSITIONS for row in got) < len(got) - 1
                    assert min(row["lowCoveragePositions"] for row in got) == 0
    finally:
        engine.close()
