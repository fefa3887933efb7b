"""Sample: the filter expression that selects a seeded random subset of its child's rows (K19), through JSON and the engine, on the
example data set as one partition and as three.  The expected rows come from tests/sample_reference.py over the data set's row
order — the same for every partitioning — with date ranges worked out here from the dates the engine's own Details returns.  Every
comparison is an exact equality."""
import calendar
import datetime

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import sample_reference as ref  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, _build_example_engine, _key_is  # noqa: E402
from tests.test_distance_matrix_gpu import example, example_data  # noqa: E402,F401  (fixtures)
from tests.test_within_distance_gpu import KEY, _check_selection, _count_of, _keys_of  # noqa: E402

EVERYTHING = {"type": "True"}
SEEDS = [0, 1, 2 ** 32 + 7]


def _sample(child, size, seed=None, **fields):
    expression = dict(fields, type="Sample", child=child, size=size)
    if seed is not None:
        expression["seed"] = seed
    return expression


def _mask(engine, data, expression):
    """The rows of the data set an expression without Sample selects, as the engine answers it (those are tested elsewhere)."""
    keys = _keys_of(engine, expression)
    return np.array([key in keys for key in data["keys"]])


def _within(data):
    return {"type": "WithinDistance", "primaryKey": data["keys"][40], "maxDistance": 30}


def _dates(engine, data, field):
    """The date of every row of the data set as the engine returns it: 'YYYY-MM-DD' or None."""
    rows = engine.execute_query({"action": {"type": "Details", "fields": [KEY, field]}, "filterExpression": EVERYTHING})
    by_key = {row[KEY]: row[field] for row in rows}
    return [by_key[key] for key in data["keys"]]


def _weekly(dates):
    """Weeks from the earliest date on, every third one left out, the last one open-ended."""
    days = sorted(datetime.date.fromisoformat(date) for date in dates if date)
    ranges, start, week = [], days[0], 0
    while start + datetime.timedelta(6) < days[-1]:
        if week % 3 != 1:
            ranges.append({"dateFrom": str(start), "dateTo": str(start + datetime.timedelta(6))})
        start, week = start + datetime.timedelta(7), week + 1
    return ranges + [{"dateFrom": str(start)}]


def _monthly(dates):
    """The calendar months that occur, newest first, without the second one; the oldest open at its start."""
    months = sorted({date[:7] for date in dates if date})
    ranges = []
    for month in months:
        year, number = int(month[:4]), int(month[5:7])
        ranges.append({"dateFrom": f"{month}-01", "dateTo": f"{month}-{calendar.monthrange(year, number)[1]:02d}"})
    ranges[0] = {"dateFrom": None, "dateTo": ranges[0]["dateTo"]}
    if len(ranges) >= 3:
        del ranges[1]
    return ranges[::-1]


def _groups(dates, ranges):
    """The range of every row (ISO dates order as strings): ref.NO_GROUP for a NULL date or a date in no range."""
    groups = np.full(len(dates), ref.NO_GROUP, dtype=np.uint16)
    for row, date in enumerate(dates):
        for index, span in enumerate(ranges):
            if date and (span.get("dateFrom") is None or span["dateFrom"] <= date) and (span.get("dateTo") is None or date <= span["dateTo"]):
                assert groups[row] == ref.NO_GROUP  # the ranges are disjoint
                groups[row] = index
    return groups


def test_sample_of_a_child_matches_the_reference(example):
    engine, oracle_db, data, partition_sizes = example
    lineage = _mask(engine, data, LINEAGE)
    from_oracle = {row[KEY] for row in so.execute_query(oracle_db, {"action": {"type": "Details", "fields": [KEY]}, "filterExpression": LINEAGE})}
    assert {data["keys"][row] for row in np.flatnonzero(lineage)} == from_oracle and 10 < lineage.sum() < len(lineage) - 10
    near = _mask(engine, data, _within(data))
    assert 5 < near.sum() < len(near) and (near != lineage).any()
    for child, selected in ((EVERYTHING, np.ones(len(data["keys"]), dtype=bool)), (LINEAGE, lineage), (_within(data), near)):
        cardinality = int(selected.sum())
        for seed in SEEDS:
            for size in (0, 1, 10, cardinality, cardinality + 5):
                want = ref.select(seed, size, selected)
                assert want.sum() == min(size, cardinality)
                _check_selection(engine, data, partition_sizes, _sample(child, size, seed), want, (child["type"], seed, size))
    # the default seed is 0; seeds give different samples
    _check_selection(engine, data, partition_sizes, _sample(LINEAGE, 10), ref.select(0, 10, lineage), "default seed")
    assert len({tuple(np.flatnonzero(ref.select(seed, 10, lineage))) for seed in SEEDS}) == len(SEEDS)
    if partition_sizes is not None:  # not vacuous: the sample of 10 of all rows has rows of more than one partition
        assert len({int(np.searchsorted(np.cumsum(partition_sizes), row, side="right")) for row in np.flatnonzero(ref.select(0, 10, np.ones(100, dtype=bool)))}) >= 2


@pytest.mark.parametrize("field", ["date", "unsorted_date"])
def test_sample_per_date_range(example, field):
    engine, _, data, partition_sizes = example
    dates = _dates(engine, data, field)
    lineage = _mask(engine, data, LINEAGE)
    everything = np.ones(len(dates), dtype=bool)
    for name, ranges in (("weekly", _weekly(dates)), ("monthly", _monthly(dates))):
        groups = _groups(dates, ranges)
        sizes = np.bincount(groups[groups != ref.NO_GROUP], minlength=len(ranges))
        # not vacuous: rows outside every range, an open-ended range with rows, strata below and above the sizes asked for
        assert (groups == ref.NO_GROUP).any() and (sizes > 0).sum() >= 2 and sizes.max() > 3 and sizes[sizes > 0].min() < 3
        open_ended = [index for index, span in enumerate(ranges) if span.get("dateFrom") is None or span.get("dateTo") is None]
        assert len(open_ended) == 1 and sizes[open_ended[0]] > 0
        for child, selected in ((EVERYTHING, everything), (LINEAGE, lineage)):
            for seed in (0, 7):
                for size in (1, 3, 100):
                    want = ref.select(seed, size, selected, groups)
                    assert want.sum() == np.minimum(np.bincount(groups[selected & (groups != ref.NO_GROUP)], minlength=len(ranges)), size).sum()
                    expression = _sample(child, size, seed, dateField=field, dateRanges=ranges)
                    _check_selection(engine, data, partition_sizes, expression, want, (name, child["type"], seed, size))
    _check_selection(engine, data, partition_sizes, _sample(EVERYTHING, 5, 1, dateField=field, dateRanges=[]), np.zeros(len(dates), dtype=bool), "no ranges")


def test_composition_with_other_expressions(example):
    engine, _, data, partition_sizes = example
    n = len(data["keys"])
    everything = np.ones(n, dtype=bool)
    lineage = _mask(engine, data, LINEAGE)
    first, second = ref.select(3, 30, everything), ref.select(4, 12, lineage)
    a, b = _sample(EVERYTHING, 30, 3), _sample(LINEAGE, 12, 4)
    assert (first & lineage).any() and (first & ~lineage).any() and (second & ~first).any()
    cases = [
        ({"type": "And", "children": [a, LINEAGE]}, first & lineage),
        ({"type": "And", "children": [LINEAGE, {"type": "Not", "child": a}]}, lineage & ~first),
        ({"type": "Or", "children": [a, b]}, first | second),
        ({"type": "And", "children": [a, b]}, first & second),
        ({"type": "Not", "child": a}, ~first),
        ({"type": "Not", "child": {"type": "Or", "children": [a, b]}}, ~(first | second)),
        ({"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [a, b, LINEAGE]}, first.astype(int) + second + lineage >= 2),
        ({"type": "Maybe", "child": a}, first),
        ({"type": "Exact", "child": b}, second),
        ({"type": "Not", "child": {"type": "Maybe", "child": b}}, ~second),
        (_sample(b, 5, 2), ref.select(2, 5, second)),                                     # a sample of a sample
        (_sample({"type": "Not", "child": a}, 9, 5), ref.select(5, 9, ~first)),
        (_sample({"type": "And", "children": [a, LINEAGE]}, 4, 6), ref.select(6, 4, first & lineage)),
        (_sample({"type": "False"}, 4, 6), np.zeros(n, dtype=bool)),
    ]
    for expression, mask in cases:
        _check_selection(engine, data, partition_sizes, expression, mask, expression["type"])
    assert 0 < (~first).sum() < n


def test_a_sample_under_maybe_takes_its_child_in_that_mode(example):
    """The child is compiled in the mode Sample is compiled in: under Maybe an ambiguous symbol matches."""
    engine, _, data, partition_sizes = example
    position = next(
        (p for p in range(1, 400) if _count_of(engine, {"type": "Maybe", "child": {"type": "NucleotideEquals", "position": p, "symbol": "A"}})
         > _count_of(engine, {"type": "NucleotideEquals", "position": p, "symbol": "A"})), None)
    assert position is not None  # a position where some row holds an ambiguity code that may be A
    child = {"type": "NucleotideEquals", "position": position, "symbol": "A"}
    exact, maybe = _mask(engine, data, child), _mask(engine, data, {"type": "Maybe", "child": child})
    assert (exact != maybe).any()
    cardinality = int(maybe.sum())
    _check_selection(engine, data, partition_sizes, {"type": "Maybe", "child": _sample(child, cardinality, 1)}, maybe, "maybe")
    _check_selection(engine, data, partition_sizes, _sample(child, cardinality, 1), exact, "exact")
    _check_selection(engine, data, partition_sizes, {"type": "Maybe", "child": _sample(child, 7, 1)}, ref.select(1, 7, maybe), "maybe, 7")


def test_actions_under_a_sample_equal_those_under_its_keys(example):
    engine, _, data, _ = example
    lineage = _mask(engine, data, LINEAGE)
    rows = np.flatnonzero(ref.select(9, 12, lineage))
    assert len(rows) == 12
    actions = [
        {"type": "Mutations", "minProportion": 0.05, "orderByFields": ["mutation"]},
        {"type": "AminoAcidMutations", "sequenceName": "S", "minProportion": 0.05, "orderByFields": ["mutation"]},
        {"type": "DistanceMatrix"},
        {"type": "Aggregated", "groupByFields": ["pango_lineage"], "orderByFields": ["pango_lineage"]},
    ]
    for action in actions:
        got = engine.execute_query({"action": action, "filterExpression": _sample(LINEAGE, 12, 9)})
        want = engine.execute_query({"action": action, "filterExpression": _key_is(data, *rows)})
        assert got == want and got, action["type"]


def test_samples_are_nested_in_their_size(example):
    engine, _, data, _ = example
    dates = _dates(engine, data, "date")
    for fields in ({}, {"dateField": "date", "dateRanges": _weekly(dates)}):
        smaller = set()
        for size in (1, 2, 3, 10, 11, 50, 100):
            larger = _keys_of(engine, _sample(EVERYTHING, size, 5, **fields))
            assert smaller <= larger and (len(larger) == size or fields), (size, list(fields))
            assert len(larger) > len(smaller) or size > 3  # (with date ranges: only while some week still has more rows)
            smaller = larger
        assert _keys_of(engine, _sample(EVERYTHING, 10, 5, **fields)) == _keys_of(engine, _sample(EVERYTHING, 10, 5, **fields))


def test_batch_of_counts_answers_as_single_queries(example):
    engine, _, data, _ = example
    dates = _dates(engine, data, "date")
    filters = [
        _sample(EVERYTHING, 17, 1),
        {"type": "And", "children": [LINEAGE, _sample(EVERYTHING, 40, 2)]},
        _sample(LINEAGE, 3, 3, dateField="date", dateRanges=_monthly(dates)),
        {"type": "Not", "child": _sample(_within(data), 4)},
        LINEAGE,
        EVERYTHING,
    ]
    queries = [{"action": {"type": "Aggregated"}, "filterExpression": expression} for expression in filters]
    singles = [engine.execute_query(query) for query in queries]
    batch = engine.execute_batch(queries)
    assert [status for status, _ in batch] == [200] * 6
    assert [document["queryResult"] for _, document in batch] == singles
    assert singles[0][0]["count"] == 17 and singles[3][0]["count"] == len(data["keys"]) - 4
    assert len({single[0]["count"] for single in singles}) > 3


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _, _ = example
    ok = _sample(EVERYTHING, 3, 1)
    week = {"dateFrom": "2021-01-04", "dateTo": "2021-01-10"}
    cases = [
        ({"type": "Sample", "size": 3}, "child"),
        (dict(ok, child="True"), "child"),
        ({"type": "Sample", "child": EVERYTHING}, "size"),
        (dict(ok, size=-1), "size"),
        (dict(ok, size=2.5), "size"),
        (dict(ok, size=2 ** 31), "size"),
        (dict(ok, seed=-1), "seed"),
        (dict(ok, seed=2 ** 63), "seed"),
        (dict(ok, dateField="date"), "dateRanges"),
        (dict(ok, dateRanges=[week]), "dateField"),
        (dict(ok, dateField="date", dateRanges=week), "dateRanges"),
        (dict(ok, dateField="date", dateRanges=[week, week]), "overlap"),
        (dict(ok, dateField="date", dateRanges=[{"dateFrom": "2021-13-01"}]), "dateFrom"),
        (dict(ok, dateField="region", dateRanges=[week]), "dateField"),
        (dict(ok, dateField="nosuchcolumn", dateRanges=[week]), "dateField"),
    ]
    for expression, named in cases:
        for wrapped in (expression, {"type": "And", "children": [LINEAGE, {"type": "Not", "child": expression}]}):
            status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": wrapped})
            assert status == 400, (expression, document)
            assert document["error"] == "Bad request" and named in document["message"] and "Sample" in document["message"], (named, document)


@pytest.mark.parametrize("by_position", [False, True], ids=["sequence-shard", "position-shard"])
def test_sharded_engine_refuses(built, example_data, by_position):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, by_position)
        status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": _sample(EVERYTHING, 3)})
        assert status == 400 and "sharded" in document["message"] and "Sample" in document["message"], document
    finally:
        engine.close()
