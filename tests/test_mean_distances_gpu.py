"""MeanDistances / AminoAcidMeanDistances: the sums of the pairwise distances within and between up to 64 named groups under the
query's filter in up to 256 regions, from the exact Mutations scan of the groups and the sums over their tables on the device (K24),
through JSON and the engine: against the numpy reference of tests/mean_distances_reference.py applied to the strings the oracle's
FastaAligned returns, against the sums of the engine's own DistanceMatrix rows (which share no kernel with K24), and on synthetic
stores in every adaptive layout against the reference on the raw symbol matrix.  Every comparison is an exact equality, doubles
included.

The groups are B.1.1.7 with its sublineages, 51 of the 100 rows, and the other 49; that they differ, that the genome and some of its
genes carry fixed differences between them and that their segregating sites are neither none nor all is asserted of the reference by
tests/test_mean_distances_reference.py without a GPU, and of the reference's rows again here before they are compared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dataset  # noqa: E402
from tests.consensus_reference import count_table  # noqa: E402
from tests.mean_distances_reference import MAX_ROWS, rows  # noqa: E402
from tests.mutations_comparison_reference import group_tables  # noqa: E402
from tests.pair_distances_reference import NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_consensus_gpu import _chars  # noqa: E402  (the cache of the oracle's strings is shared)
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mean_distances_reference import GENES  # noqa: E402
from tests.test_mutations_comparison_gpu import _mask  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"region", "positionFrom", "positionTo", "sequenceName", "group", "otherGroup", "count", "otherCount", "pairs", "differences",
          "comparedPositions", "segregatingSites", "fixedDifferences", "meanDistance", "meanCompared", "distancePerSite"}
ORDERABLE = ["region", "positionFrom", "positionTo", "group", "otherGroup", "count", "otherCount", "segregatingSites", "fixedDifferences",
             "meanDistance", "meanCompared", "distancePerSite"]
SEQUENCES = [(None, "main", "nuc"), ("S", "S", "aa")]  # (sequenceName of the request, the store, its alphabet)
TRUE = {"type": "True"}
FALSE = {"type": "False"}
OTHERS = {"type": "Not", "child": LINEAGE}
DATES = {"type": "DateBetween", "column": "date", "from": "2021-01-01", "to": "2021-03-31"}
TWO = [("lineage", LINEAGE), ("others", OTHERS)]
# overlapping regions in shuffled order, a single position, the first and the last position
MIXED = [("late", 20000, 29903), ("one", 23403, 23403), ("early", 1, 21000), ("middle", 15000, 25000), ("first", 1, 1), ("last", 29903, 29903)]
PAST_THE_END = "{}: the region '{}': positionTo {} is past the end of the sequence '{}' ({} positions)"
ROW_CAP = "{} action: {} regions x {} pairs of groups are {} rows, more than the 65536 a response may hold"
SHARDED = "{} is not supported on a sharded database yet: its counts are not all-reduced across ranks"


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


def _want(oracle_db, data, store, alphabet, query_filter, groups=None, regions=None, between=True):
    chars = _chars(oracle_db, store, TRUE)[1]
    base = _mask(oracle_db, data, store, query_filter)
    masks = [base] if groups is None else [base & _mask(oracle_db, data, store, expression) for _, expression in groups]
    tables = group_tables([chars[mask] for mask in masks], alphabet, chars.shape[1])
    names = [None] if groups is None else [name for name, _ in groups]
    return rows(tables, [int(mask.sum()) for mask in masks], names, [(None, 1, chars.shape[1])] if regions is None else regions, store, between)


def _action(sequence_name, alphabet, groups=None, regions=None, **fields):
    action = dict(fields, type="MeanDistances" if alphabet == "nuc" else "AminoAcidMeanDistances")
    if groups is not None:
        action["groups"] = [{"name": name, "filterExpression": expression} for name, expression in groups]
    if regions is not None:
        action["regions"] = [{"name": name, "positionFrom": first, "positionTo": last} for name, first, last in regions]
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _regions_of(store):
    return {"main": [None, GENES, MIXED], "S": [None, [("rbd", 319, 541), ("one", 614, 614), ("all", 1, 1274), ("start", 1, 400)]]}[store]


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        for regions in _regions_of(store):
            want = _want(oracle_db, data, store, alphabet, TRUE, TWO, regions)
            within = [row for row in want if row["group"] == row["otherGroup"]]
            between = [row for row in want if row["group"] != row["otherGroup"]]
            assert len(want) == 3 * len(regions or [None]) and (within[0]["count"], within[1]["count"]) == (51, 49)
            if regions is None:  # the reference itself: the groups differ
                assert int(between[0]["differences"]) > 0 and 0 < within[0]["segregatingSites"] < within[0]["positionTo"]
                assert (between[0]["fixedDifferences"] > 0) == (store == "main")
            if regions is GENES:
                assert sum(row["fixedDifferences"] > 0 for row in between) >= 2 and any(row["fixedDifferences"] == 0 for row in between)
            got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO, regions), "filterExpression": TRUE})
            assert got == want, (store, regions)
            assert all(set(row) == FIELDS for row in got)
            for row in got:  # the doubles: the correctly rounded integers, one division
                differences, compared, pairs = int(row["differences"]), int(row["comparedPositions"]), int(row["pairs"])
                assert row["meanDistance"] == float(differences) / float(pairs) and row["meanCompared"] == float(compared) / float(pairs)
                assert row["distancePerSite"] == (float(differences) / float(compared) if compared else None)


def test_the_sums_of_the_engines_own_distance_matrix(example):
    """DistanceMatrix compares rows with rows (K10): its `distance` and `comparedPositions` summed over the rectangle of two disjoint
    groups and over the pairs i < j of each.  Of two groups that share rows the rectangle counts a pair of two shared rows twice and
    a shared row with itself (distance 0): the differences are compared."""
    engine, _, data = example
    overlap = [("a", _key_is(data, 40, 3, 99, 57, 38, 12)), ("b", _key_is(data, 3, 12, 60, 37, 57, 5, 0))]
    for sequence_name, store, alphabet in SEQUENCES:
        matrix = engine.execute_query({"action": dict({"type": "DistanceMatrix"}, **({"sequenceName": sequence_name} if sequence_name else {})), "filterExpression": TRUE})
        keys = {}
        for name, expression in TWO + overlap:
            selected = engine.execute_query({"action": {"type": "Details", "fields": ["gisaid_epi_isl"]}, "filterExpression": expression})
            keys[name] = {row["gisaid_epi_isl"] for row in selected}
        assert (len(keys["lineage"]), len(keys["others"]), len(keys["a"] & keys["b"])) == (51, 49, 3)

        def summed(first, second, field):  # over the ordered pairs (i in first, j in second), i != j
            return sum(row[field] * ((row["firstKey"] in first and row["secondKey"] in second) + (row["secondKey"] in first and row["firstKey"] in second))
                       for row in matrix)

        got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO), "filterExpression": TRUE})
        for row in got:
            first, second = keys[row["group"]], keys[row["otherGroup"]]
            halved = 2 if row["group"] == row["otherGroup"] else 1  # the unordered pairs of one group
            assert int(row["differences"]) == summed(first, second, "distance") // halved > 0, (store, row["group"], row["otherGroup"])
            assert int(row["comparedPositions"]) == summed(first, second, "comparedPositions") // halved
        got = engine.execute_query({"action": _action(sequence_name, alphabet, overlap), "filterExpression": TRUE})
        assert [int(row["differences"]) for row in got] == [summed(keys["a"], keys["a"], "distance") // 2, summed(keys["a"], keys["b"], "distance"),
                                                            summed(keys["b"], keys["b"], "distance") // 2]
        assert got[1]["pairs"] == "42" and int(got[1]["comparedPositions"]) > summed(keys["a"], keys["b"], "comparedPositions")  # the three rows with themselves


def test_without_groups_is_one_group_of_every_row(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        for query_filter in (TRUE, LINEAGE):
            got = engine.execute_query({"action": _action(sequence_name, alphabet), "filterExpression": query_filter})
            assert got == _want(oracle_db, data, store, alphabet, query_filter) and len(got) == 1
            assert got[0]["group"] is None and got[0]["otherGroup"] is None and got[0]["region"] is None and got[0]["fixedDifferences"] is None
            named = engine.execute_query({"action": _action(sequence_name, alphabet, [("all", TRUE)]), "filterExpression": query_filter})
            assert named == [dict(got[0], group="all", otherGroup="all")] and int(got[0]["differences"]) > 0


def test_overlapping_identical_and_empty_groups(example):
    engine, oracle_db, data = example
    groups = [("all", TRUE), ("lineage", LINEAGE), ("none", FALSE), ("again", {"type": "And", "children": [LINEAGE, TRUE]}),
              ("spanning", _key_is(data, 40, 3, 99, 57, 38)), ("one", _key_is(data, 37)), ("others", OTHERS), ("overlap", _key_is(data, 40, 3, 12, 60, 37)),
              ("first", _key_is(data, 5, 30, 36, 0))]  # more than one scan batch
    for sequence_name, store, alphabet in SEQUENCES:
        for query_filter in (TRUE, LINEAGE):  # a group ANDs with the query's filter
            got = engine.execute_query({"action": _action(sequence_name, alphabet, groups), "filterExpression": query_filter})
            assert got == _want(oracle_db, data, store, alphabet, query_filter, groups) and len(got) == 45
            of = {(row["group"], row["otherGroup"]): row for row in got}
            assert [row["group"] for row in got[:9]] == ["all"] * 9 and [row["otherGroup"] for row in got[:9]] == [name for name, _ in groups]
            same = of[("lineage", "again")]  # identical groups: every row with every row, itself included
            assert same["pairs"] == "2601" and int(same["differences"]) == 2 * int(of[("lineage", "lineage")]["differences"]) > 0
            for pair, row in of.items():
                if "none" in pair:  # an empty group
                    assert row["pairs"] == "0" and row["differences"] == "0" and row["comparedPositions"] == "0"
                    assert row["meanDistance"] is None and row["meanCompared"] is None and row["distancePerSite"] is None
            assert of[("none", "none")]["count"] == 0 and of[("none", "none")]["segregatingSites"] == 0 and of[("all", "none")]["fixedDifferences"] == 0
            assert of[("one", "one")]["pairs"] == "0" and of[("one", "one")]["meanDistance"] is None
        got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO, _regions_of(store)[1]), "filterExpression": FALSE})  # an empty selection
        assert got == _want(oracle_db, data, store, alphabet, FALSE, TWO, _regions_of(store)[1])
        assert got and all(row["pairs"] == "0" and row["count"] == 0 and row["meanDistance"] is None for row in got)


def test_between_false_keeps_the_rows_within(example):
    engine, oracle_db, data = example
    groups = TWO + [("spanning", _key_is(data, 40, 3, 99, 57, 38))]
    for sequence_name, store, alphabet in SEQUENCES:
        regions = _regions_of(store)[1]
        whole = engine.execute_query({"action": _action(sequence_name, alphabet, groups, regions, between=True), "filterExpression": TRUE})
        within = engine.execute_query({"action": _action(sequence_name, alphabet, groups, regions, between=False), "filterExpression": TRUE})
        assert within == [row for row in whole if row["group"] == row["otherGroup"]] == _want(oracle_db, data, store, alphabet, TRUE, groups, regions, between=False)
        assert len(within) == 3 * len(regions) and len(whole) == 6 * len(regions)


def test_under_a_base_filter(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        base = _mask(oracle_db, data, store, DATES)
        lineage = _mask(oracle_db, data, store, LINEAGE)
        assert 0 < (base & lineage).sum() < lineage.sum() and 0 < (base & ~lineage).sum() < (~lineage).sum()
        for regions in _regions_of(store):
            got = engine.execute_query({"action": _action(sequence_name, alphabet, TWO, regions), "filterExpression": DATES})
            assert got == _want(oracle_db, data, store, alphabet, DATES, TWO, regions)
            assert got[0]["count"] == (base & lineage).sum() and int(got[1]["differences"]) > 0


def _sort_key(field):
    return lambda row: (row[field] is not None, row[field] if row[field] is not None else 0)


def test_order_limit_offset(example):
    engine, _, data = example
    groups = [("lineage", LINEAGE), ("none", FALSE), ("others", OTHERS)]
    for sequence_name, store, alphabet in SEQUENCES:
        base = _action(sequence_name, alphabet, groups, _regions_of(store)[1])
        got = engine.execute_query({"action": base, "filterExpression": TRUE})
        assert len(got) >= 24
        unique = sorted(got, key=lambda row: (row["region"], row["group"], row["otherGroup"]))
        for field in ORDERABLE:
            for descending in (False, True):
                order_by = [{"field": field, "order": "descending" if descending else "ascending"}, "region", "group", "otherGroup"]
                want = sorted(unique, key=_sort_key(field), reverse=descending)  # (stable: ties stay by region, group, otherGroup)
                for limit, offset in ((4, 2), (10_000, 0), (5, len(got) - 3)):
                    ordered = engine.execute_query({"action": dict(base, orderByFields=order_by, limit=limit, offset=offset), "filterExpression": TRUE})
                    assert ordered == want[offset:offset + limit], (field, descending, limit, offset)
            # something to put in order (no amino acid of S is fixed between the groups: null and 0)
            assert len({row[field] for row in got}) >= (2 if (store, field) == ("S", "fixedDifferences") else 3)
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": TRUE}) == got[2:6]  # of the rows in request order
        assert engine.execute_query({"action": dict(base, offset=len(got)), "filterExpression": TRUE}) == []


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _ = example
    a, b = {"name": "a", "filterExpression": TRUE}, {"name": "b", "filterExpression": LINEAGE}
    region = {"name": "r", "positionFrom": 1, "positionTo": 10}
    ok = {"type": "MeanDistances", "groups": [a, b], "regions": [region]}
    aa = {"type": "AminoAcidMeanDistances", "sequenceName": "S", "groups": [a, b], "regions": [region]}
    many = [{"name": str(g), "filterExpression": TRUE} for g in range(23)]
    cases = [
        (dict(ok, regions=[dict(region, positionTo=29904)]), PAST_THE_END.format("MeanDistances", "r", 29904, "main", 29903)),
        (dict(ok, regions=[region, dict(region, name="far", positionFrom=40000, positionTo=2147483647)]), PAST_THE_END.format("MeanDistances", "far", 2147483647, "main", 29903)),
        (dict(aa, regions=[dict(region, positionTo=1275)]), PAST_THE_END.format("AminoAcidMeanDistances", "r", 1275, "S", 1274)),
        (dict(ok, groups=many, regions=[dict(region, name=str(r)) for r in range(256)]), ROW_CAP.format("MeanDistances", 256, 276, 70656)),
        (dict(ok, groups=[b, {"name": "c", "filterExpression": {"type": "FloatBetween", "column": "nosuchcolumn", "from": 0.5, "to": 1.5}}]), "filterExpression of the group 'c'"),
        (dict(ok, sequenceName="nosuchsequence"), "'nosuchsequence'"),
        (dict(ok, sequenceName="S"), "'S'"),  # a gene is no nucleotide sequence
        (dict(aa, sequenceName="main"), "'main'"),
        ({"type": "AminoAcidMeanDistances"}, "sequenceName"),
        (dict(ok, between="yes"), "between"),
        (dict(ok, orderByFields=["pairs"]), "pairs"),
        (dict(ok, orderByFields=["sequenceName"]), "sequenceName"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
        if named.startswith(("MeanDistances", "AminoAcidMeanDistances")):
            assert document["message"] == named
    within_the_cap = dict(ok, groups=many, regions=[dict(region, name=str(r)) for r in range(237)], limit=2)  # 237 x 276 = 65 412 rows
    for action in (ok, aa, dict(ok, regions=[dict(region, positionTo=29903)]), dict(aa, regions=[dict(region, positionFrom=1274, positionTo=1274)]), within_the_cap,
                   dict(ok, groups=many, regions=[dict(region, name=str(r)) for r in range(256)], between=False, limit=3),
                   dict(ok, sequenceName="testSecondSequence", regions=[dict(region, positionTo=4)]), dict(aa, sequenceName="ORF1a", orderByFields=ORDERABLE),
                   dict(ok, groups=[{"name": str(g), "filterExpression": TRUE if g else LINEAGE} for g in range(64)], limit=5, offset=2070, orderByFields=ORDERABLE)):
        status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
        assert status == 200 and document["queryResult"] and all(set(row) == FIELDS for row in document["queryResult"]), document
    assert 237 * 276 <= MAX_ROWS < 238 * 276


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        for action in ({"type": "MeanDistances"}, {"type": "AminoAcidMeanDistances", "sequenceName": "S", "groups": [{"name": "a", "filterExpression": TRUE}]}):
            status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
            assert status == 400 and document["message"] == SHARDED.format(action["type"]), document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2031)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the exact scan over derived symbols, runs of N, sparse ambiguity keys and code planes, then the sums,
    for 8 + 1 groups (a second scan batch) under the whole store (its cached totals for the group of every row) and under a lineage-like
    range of 31 001 rows.  The group of every row has 9.8e9 pairs within: sums above 2^32."""
    sym, _, bucket = synthetic
    chars = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)[sym]
    all_rows = np.arange(N_ROWS)
    in_range = (all_rows >= 30_000) & (all_rows <= 61_000)
    stretch = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}
    groups = [(f"bucket{b}", {"type": "IntBetween", "column": "bucket", "from": 100 * b, "to": 100 * b + 99 - 10 * b}, (bucket >= 100 * b) & (bucket <= 100 * b + 99 - 10 * b))
              for b in range(8)] + [("early", {"type": "IntBetween", "column": "row", "from": 0, "to": 45_000}, all_rows <= 45_000)]
    whole = [("everything", TRUE, np.ones(N_ROWS, dtype=bool)), groups[0], groups[8]]
    regions = [("all", 1, POSITIONS), ("head", 1, 17), ("tail", 16, POSITIONS), ("one", 33, 33)]
    assert NUC_VALID == "-ACGT"
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for query_filter, mask in ((TRUE, np.ones(N_ROWS, dtype=bool)), (stretch, in_range)):
            for listed in (groups, whole):
                tables = np.stack([count_table(chars[mask & group], "nuc") for _, _, group in listed])
                want = rows(tables, [int((mask & group).sum()) for _, _, group in listed], [name for name, _, _ in listed], regions, "main")
                got = engine.execute_query({"action": _action(None, "nuc", [(name, expression) for name, expression, _ in listed], regions), "filterExpression": query_filter})
                assert got == want, (layout, missing_runs, query_filter, listed[0][0])
                assert all(int(row["differences"]) > 0 for row in want if row["region"] != "one")
                assert listed is groups or query_filter is stretch or int(want[0]["differences"]) > 2**32  # of every row with every other
    finally:
        engine.close()
