"""MutationsComparison / AminoAcidMutationsComparison: how often each of 2 .. 64 named groups under the query's filter carries each
mutation that any of them carries, from the exact Mutations scan of the groups and the comparison on the device (K17), through JSON and
the engine: against the numpy reference of tests/mutations_comparison_reference.py applied to the strings the oracle's FastaAligned
returns, against the engine's own Mutations rows of every group, and on synthetic stores in every adaptive layout against the reference
on the raw symbol matrix.  Every comparison is an exact equality, doubles included.

The numbers of mutations that the tests assert of the reference before they compare (main = the default nucleotide sequence, 29 903
positions; S = the gene, 1 274; the groups are B.1.1.7 with its sublineages, 51 of the 100 rows, and the other 49) were worked out on
the CPU with the oracle.  Main's 1 441 mutations at (0, 0) are more than the 1 024 records of the first comparison: the second runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dataset  # noqa: E402
from tests.consensus_reference import count_table  # noqa: E402
from tests.mutations_comparison_reference import FIRST_CAPACITY, comparison_rows, group_tables  # noqa: E402
from tests.pair_distances_reference import NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_consensus_gpu import _chars, _reference_of  # noqa: E402  (the cache of the oracle's strings is shared)
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"mutation", "sequenceName", "position", "group", "count", "coverage", "proportion", "difference"}
ORDERABLE = ["mutation", "position", "group", "count", "coverage", "proportion", "difference"]
SEQUENCES = [(None, "main", "nuc"), ("S", "S", "aa")]  # (sequenceName of the request, the store, its alphabet)
TRUE = {"type": "True"}
FALSE = {"type": "False"}
OTHERS = {"type": "Not", "child": LINEAGE}
DATES = {"type": "DateBetween", "column": "date", "from": "2021-01-01", "to": "2021-03-31"}
TWO = [("lineage", LINEAGE), ("others", OTHERS)]
# (minProportion, minDifference) -> the mutations the reference selects for TWO under no filter
SELECTED = {"main": {(0.05, 0.0): 517, (0.05, 0.5): 43, (0.5, 0.0): 114, (1.0, 0.0): 26, (0.0, 0.0): 1441},
            "S": {(0.05, 0.0): 61, (0.05, 0.5): 0, (0.05, 0.25): 2}}


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


def _mask(oracle_db, data, store, expression):
    """bool [100]: the rows of the data set that `expression` selects.  True, False, And, Not and an Or of primary keys are worked out
    here; everything else is what the oracle's FastaAligned returns for it (asked once per store and expression)."""
    keys = _chars(oracle_db, store, TRUE)[0]
    kind = expression["type"]
    if kind == "True":
        return np.ones(len(keys), dtype=bool)
    if kind == "False":
        return np.zeros(len(keys), dtype=bool)
    if kind == "Not":
        return ~_mask(oracle_db, data, store, expression["child"])
    if kind == "And":
        return np.logical_and.reduce([_mask(oracle_db, data, store, child) for child in expression["children"]])
    if kind == "Or" and all(child["type"] == "StringEquals" for child in expression["children"]):
        return np.logical_or.reduce([_mask(oracle_db, data, store, child) for child in expression["children"]])
    if kind == "StringEquals" and expression["column"] == "gisaid_epi_isl":
        return np.array([key == expression["value"] for key in keys])
    selected = set(_chars(oracle_db, store, expression)[0])
    return np.array([key in selected for key in keys])


def _tables(oracle_db, data, store, alphabet, query_filter, groups):
    chars = _chars(oracle_db, store, TRUE)[1]
    base = _mask(oracle_db, data, store, query_filter)
    return group_tables([chars[base & _mask(oracle_db, data, store, expression)] for _, expression in groups], alphabet, chars.shape[1])


def _want(oracle_db, data, store, alphabet, query_filter, groups, min_proportion=0.05, min_difference=0.0):
    tables = _tables(oracle_db, data, store, alphabet, query_filter, groups)
    return comparison_rows(tables, _reference_of(data, store, alphabet), alphabet, store, [name for name, _ in groups], min_proportion, min_difference)


def _action(sequence_name, alphabet, groups, **fields):
    action = dict(fields, type="MutationsComparison" if alphabet == "nuc" else "AminoAcidMutationsComparison",
                  groups=[{"name": name, "filterExpression": expression} for name, expression in groups])
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _passes(row, min_proportion):
    """Whether the group of a response row passes the row's mutation: K4's bound, from the row's own count and coverage."""
    if row["coverage"] == 0:
        return False
    bound = 0 if min_proportion == 0 else int(np.ceil(np.float64(row["coverage"]) * np.float64(min_proportion)) - 1)
    return row["count"] > bound


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        for (min_proportion, min_difference), selected in SELECTED[store].items():
            want = _want(oracle_db, data, store, alphabet, TRUE, TWO, min_proportion, min_difference)
            case = (store, min_proportion, min_difference)
            assert len(want) == 2 * selected, (case, len(want) // 2)  # the reference itself
            if case == ("main", 0.05, 0.5):
                mutations = [want[k:k + 2] for k in range(0, len(want), 2)]
                assert sum(not all(_passes(row, min_proportion) for row in rows) for rows in mutations) == 33
            if case == ("main", 0.0, 0.0):
                assert selected > FIRST_CAPACITY  # the first comparison's records do not hold them
            got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO, minProportion=min_proportion, minDifference=min_difference),
                                        "filterExpression": TRUE})
            assert got == want, case
            assert all(set(row) == FIELDS for row in got)
        default = engine.execute_query({"action": _action(sequence_name, alphabet, TWO), "filterExpression": TRUE})
        assert default == _want(oracle_db, data, store, alphabet, TRUE, TWO, 0.05, 0.0)  # the defaults
        coverages = {(row["group"], row["coverage"]) for row in default}
        assert max(c for g, c in coverages if g == "lineage") == 51 and max(c for g, c in coverages if g == "others") == 49


def test_under_a_base_filter(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        base = _mask(oracle_db, data, store, DATES)
        lineage = _mask(oracle_db, data, store, LINEAGE)
        assert 0 < (base & lineage).sum() < lineage.sum() and 0 < (base & ~lineage).sum() < (~lineage).sum()
        for min_proportion, min_difference in ((0.05, 0.0), (0.05, 0.3), (0.0, 0.0)):
            want = _want(oracle_db, data, store, alphabet, DATES, TWO, min_proportion, min_difference)
            got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO, minProportion=min_proportion, minDifference=min_difference),
                                        "filterExpression": DATES})
            assert got == want and want, (store, min_proportion, min_difference)
            assert max(row["coverage"] for row in got if row["group"] == "lineage") == (base & lineage).sum()


def test_the_rows_a_group_passes_are_its_own_mutations_rows(example):
    engine, _, _ = example
    for sequence_name, store, alphabet in SEQUENCES:
        mutations_type = "Mutations" if alphabet == "nuc" else "AminoAcidMutations"
        for query_filter in (TRUE, DATES):
            for min_proportion in (0.05, 0.5, 0.0):
                got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO, minProportion=min_proportion, minDifference=0), "filterExpression": query_filter})
                for name, expression in TWO:
                    both = {"type": "And", "children": [query_filter, expression]}
                    own = engine.execute_query({"action": {"type": mutations_type, "sequenceName": store, "minProportion": min_proportion}, "filterExpression": both})
                    passed = {row["mutation"]: (row["count"], row["proportion"]) for row in got if row["group"] == name and _passes(row, min_proportion)}
                    assert passed == {row["mutation"]: (row["count"], row["proportion"]) for row in own} and own, (store, query_filter, min_proportion, name)


def test_identical_and_empty_groups(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        same = [("a", LINEAGE), ("b", {"type": "And", "children": [LINEAGE, TRUE]})]
        assert engine.execute_query({"action": _action(sequence_name, alphabet, same, minDifference=0.01), "filterExpression": TRUE}) == []
        got = engine.execute_query({"action": _action(sequence_name, alphabet, same), "filterExpression": TRUE})
        assert got == _want(oracle_db, data, store, alphabet, TRUE, same) and got and {row["difference"] for row in got} == {0.0}
        with_empty = [("lineage", LINEAGE), ("none", FALSE), ("others", OTHERS)]
        got = engine.execute_query({"action": _action(sequence_name, alphabet, with_empty), "filterExpression": TRUE})
        assert got == _want(oracle_db, data, store, alphabet, TRUE, with_empty)
        of_none = [row for row in got if row["group"] == "none"]
        assert len(of_none) * 3 == len(got) > 0 and all(row["count"] == 0 and row["coverage"] == 0 and row["proportion"] is None for row in of_none)
        assert [row["group"] for row in got[:3]] == ["lineage", "none", "others"]  # in the order of the request
        nobody = [("none", FALSE), ("nothing", {"type": "And", "children": [LINEAGE, OTHERS]})]
        for query_filter in (TRUE, FALSE):
            assert engine.execute_query({"action": _action(sequence_name, alphabet, nobody, minProportion=0), "filterExpression": query_filter}) == []
        assert engine.execute_query({"action": _action(sequence_name, alphabet, TWO, minProportion=0), "filterExpression": FALSE}) == []


def _nine_groups(data):
    """More than one scan batch; `none` selects nothing, `lineage` and `again` the same rows, `spanning` and `overlap` share rows."""
    return [("all", TRUE), ("lineage", LINEAGE), ("spanning", _key_is(data, 40, 3, 99, 57, 38)), ("one", _key_is(data, 37)), ("none", FALSE),
            ("again", {"type": "And", "children": [LINEAGE, TRUE]}), ("others", OTHERS), ("overlap", _key_is(data, 40, 3, 12, 60, 37)),
            ("first", _key_is(data, 5, 30, 36, 0))]


def test_nine_groups_match_the_reference(example):
    engine, oracle_db, data = example
    groups = _nine_groups(data)
    for sequence_name, store, alphabet in SEQUENCES:
        for query_filter in (TRUE, LINEAGE):  # a group ANDs with the query's filter
            for min_proportion, min_difference in ((0.05, 0.0), (0.5, 0.5)):
                got = engine.execute_query({"action": _action(sequence_name, alphabet, groups, minProportion=min_proportion, minDifference=min_difference),
                                            "filterExpression": query_filter})
                assert got == _want(oracle_db, data, store, alphabet, query_filter, groups, min_proportion, min_difference), (store, query_filter, min_proportion)
                assert got and [row["group"] for row in got[:9]] == [name for name, _ in groups]


def _sort_key(field):
    return lambda row: (row[field] is not None, row[field] if row[field] is not None else 0)


def test_order_limit_offset(example):
    engine, _, data = example
    groups = [("lineage", LINEAGE), ("none", FALSE), ("others", OTHERS)]
    for sequence_name, _, alphabet in SEQUENCES:
        base = _action(sequence_name, alphabet, groups, minProportion=0.3)
        got = engine.execute_query({"action": base, "filterExpression": TRUE})
        assert len(got) >= 30
        unique = sorted(got, key=lambda row: (row["position"], row["mutation"], row["group"]))
        for field in ORDERABLE:
            for descending in (False, True):
                order_by = [{"field": field, "order": "descending" if descending else "ascending"}, "position", "mutation", "group"]
                want = sorted(unique, key=_sort_key(field), reverse=descending)  # (stable: ties stay by position, mutation, group)
                for limit, offset in ((4, 2), (10_000, 0), (5, len(got) - 3)):
                    ordered = engine.execute_query({"action": dict(base, orderByFields=order_by, limit=limit, offset=offset), "filterExpression": TRUE})
                    assert ordered == want[offset:offset + limit], (field, descending, limit, offset)
            assert len({row[field] for row in got}) >= 3  # something to put in order
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": TRUE}) == got[2:6]  # of the flat rows
        assert engine.execute_query({"action": dict(base, offset=len(got)), "filterExpression": TRUE}) == []


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _ = example
    a, b = {"name": "a", "filterExpression": TRUE}, {"name": "b", "filterExpression": LINEAGE}
    ok = {"type": "MutationsComparison", "groups": [a, b]}
    cases = [
        (dict(ok, minProportion=-0.5), "minProportion must be in interval [0.0, 1.0]"),
        (dict(ok, minProportion=1.5), "minProportion must be in interval [0.0, 1.0]"),
        (dict(ok, minProportion="0.5"), "minProportion"),
        (dict(ok, minProportion=None), "minProportion"),
        (dict(ok, minProportion=[0.5]), "minProportion"),
        (dict(ok, minDifference=-0.5), "minDifference"),
        (dict(ok, minDifference=1.5), "minDifference"),
        (dict(ok, minDifference="0.5"), "minDifference"),
        (dict(ok, minDifference=None), "minDifference"),
        (dict(ok, minDifference=[0.5]), "minDifference"),
        ({"type": "MutationsComparison"}, "groups"),
        (dict(ok, groups=a), "groups"),
        (dict(ok, groups="a"), "groups"),
        (dict(ok, groups=None), "groups"),
        (dict(ok, groups=[]), "fewer than the 2"),
        (dict(ok, groups=[a]), "fewer than the 2"),
        (dict(ok, groups=[TRUE, 5]), "groups"),
        (dict(ok, groups=[a, {"filterExpression": TRUE}]), "name"),
        (dict(ok, groups=[a, {"name": 5, "filterExpression": TRUE}]), "name"),
        (dict(ok, groups=[a, dict(a)]), "'a' occurs more than once"),
        (dict(ok, groups=[b, {"name": "a"}]), "filterExpression of the group 'a'"),
        (dict(ok, groups=[b, {"name": "a", "filterExpression": "True"}]), "filterExpression of the group 'a'"),
        (dict(ok, groups=[a, {"name": "c", "filterExpression": {"type": "NoSuchFilter"}}]), "filterExpression of the group 'c'"),
        (dict(ok, groups=[a, {"name": "c", "filterExpression": {"column": "pango_lineage"}}]), "filterExpression of the group 'c'"),
        (dict(ok, groups=[a, {"name": "c", "filterExpression": {"type": "FloatBetween", "column": "nosuchcolumn", "from": 0.5, "to": 1.5}}]), "filterExpression of the group 'c'"),
        (dict(ok, groups=[a, {"name": "c", "filterExpression": {"type": "FloatBetween", "column": "nosuchcolumn", "from": 0.5, "to": 1.5}}]), "nosuchcolumn"),
        (dict(ok, groups=[{"name": str(g), "filterExpression": TRUE} for g in range(65)]), "limit of 64"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "'nosuchsequence'"),
        (dict(ok, sequenceName="S"), "'S'"),  # a gene is no nucleotide sequence
        ({"type": "AminoAcidMutationsComparison", "groups": [a, b]}, "sequenceName"),
        ({"type": "AminoAcidMutationsComparison", "groups": [a, b], "sequenceName": "main"}, "'main'"),
        (dict(ok, orderByFields=["sequenceName"]), "sequenceName"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (ok, dict(ok, minProportion=1, minDifference=0), dict(ok, minProportion=0, minDifference=1), dict(ok, sequenceName="testSecondSequence", minProportion=0),
                   dict(ok, groups=[{"name": str(g), "filterExpression": TRUE if g else LINEAGE} for g in range(64)], minProportion=0.9, orderByFields=ORDERABLE),
                   {"type": "AminoAcidMutationsComparison", "sequenceName": "ORF1a", "groups": [a, b], "orderByFields": ORDERABLE}):
        status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
        assert status == 200 and all(set(row) == FIELDS for row in document["queryResult"]), document
        assert len(document["queryResult"]) % len(action["groups"]) == 0
        assert document["queryResult"] or action.get("minDifference") == 1 or "sequenceName" in action


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    groups = [{"name": "a", "filterExpression": TRUE}, {"name": "b", "filterExpression": LINEAGE}]
    try:
        engine.set_sharding(0, 2, False)
        for action in ({"type": "MutationsComparison", "groups": groups}, {"type": "AminoAcidMutationsComparison", "sequenceName": "S", "groups": groups}):
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
    comparison, for 8 + 1 groups (a second scan batch) under the whole store (its cached totals for the group of every row) and under a
    lineage-like range of 31 001 rows."""
    sym, _, bucket = synthetic
    reference = "".join(NUC_VALID[1 + (p % 4)] for p in range(POSITIONS))  # as _synthetic_engine gives it
    chars = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)[sym]
    rows = np.arange(N_ROWS)
    in_range = (rows >= 30_000) & (rows <= 61_000)
    stretch = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}
    groups = [(f"bucket{b}", {"type": "IntBetween", "column": "bucket", "from": 100 * b, "to": 100 * b + 99 - 10 * b}, (bucket >= 100 * b) & (bucket <= 100 * b + 99 - 10 * b))
              for b in range(8)] + [("early", {"type": "IntBetween", "column": "row", "from": 0, "to": 45_000}, rows <= 45_000)]
    whole = [("everything", TRUE, np.ones(N_ROWS, dtype=bool)), groups[0], groups[8]]
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for query_filter, mask in ((TRUE, np.ones(N_ROWS, dtype=bool)), (stretch, in_range)):
            for listed in (groups, whole):
                tables = np.stack([count_table(chars[mask & group], "nuc") for _, _, group in listed])
                names = [name for name, _, _ in listed]
                sizes = []
                for min_proportion, min_difference in ((0.05, 0.0), (0.0, 0.0), (0.01, 0.004)):
                    want = comparison_rows(tables, reference, "nuc", "main", names, min_proportion, min_difference)
                    action = _action(None, "nuc", [(name, expression) for name, expression, _ in listed], minProportion=min_proportion, minDifference=min_difference)
                    got = engine.execute_query({"action": action, "filterExpression": query_filter})
                    assert got == want, (layout, missing_runs, query_filter, names[0], min_proportion, min_difference)
                    sizes.append(len(want))
                assert 0 < sizes[0] < sizes[1] and 0 < sizes[2] < sizes[1], sizes  # not vacuous: both settings decide something
    finally:
        engine.close()

