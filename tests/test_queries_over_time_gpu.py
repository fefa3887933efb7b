"""QueriesOverTime: count and coverage per (labelled query, date range) from the grouped filter count kernel (K8), through JSON and
the engine: against row sets the oracle selects for And(filter, sub-expression) intersected with the raw dates (both ends of a
range inclusive, NULL dates in none — never through DateBetween), and on a synthetic store that mixes the adaptive layouts against
numpy on the raw symbol matrix."""
import datetime
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.test_mutations_over_time_gpu import (  # noqa: E402
    EXAMPLE_RANGES, N_ROWS, NUC_CHARS, NUC_VALID, POSITIONS, SYNTHETIC_RANGES, _build_example_engine, _day, _pick_mutations, _range_json,
    _synthetic_dates, _synthetic_matrix)
from tests.test_oracle_golden import build_oracle_db  # noqa: E402

LINEAGE = {"type": "PangoLineage", "column": "pango_lineage", "value": "B.1.1.7", "includeSublineages": True}
TOP_FILTERS = [
    {"type": "PangoLineage", "column": "pango_lineage", "value": "NO.SUCH.LINEAGE", "includeSublineages": False},  # selects no row
    LINEAGE,
    {"type": "True"},
]


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, [37, 1, 62]], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


def _selected_keys(oracle_db, expression, cache):
    text = json.dumps(expression, sort_keys=True)
    if text not in cache:
        cache[text] = {row["gisaid_epi_isl"] for row in so.execute_query(
            oracle_db, {"action": {"type": "Details", "fields": ["gisaid_epi_isl"]}, "filterExpression": expression})}
    return cache[text]


def _expected(oracle_db, data, action, top, cache):
    """Per (query, range) the rows the oracle selects for And(top, sub-expression) whose raw date lies in the range."""
    field = action["dateField"]
    dates = [so.string_to_date(row.get(field) or "") for row in data["rows"]]
    keys = [row["gisaid_epi_isl"] for row in data["rows"]]
    out = []
    for query in action["queries"]:
        selected = [_selected_keys(oracle_db, {"type": "And", "children": [top, query[which]]}, cache) for which in ("countQuery", "coverageQuery")]
        for date_range in action["dateRanges"]:
            low = so.string_to_date(date_range["dateFrom"]) if date_range.get("dateFrom") else 1
            high = so.string_to_date(date_range["dateTo"]) if date_range.get("dateTo") else 0xFFFFFFFF
            in_range = [key for key, date in zip(keys, dates) if date != 0 and low <= date <= high]
            out.append({"count": sum(key in selected[0] for key in in_range), "coverage": sum(key in selected[1] for key in in_range),
                        "dateFrom": date_range.get("dateFrom"), "dateTo": date_range.get("dateTo"), "displayLabel": query["displayLabel"]})
    return out


def _example_queries(data):
    """Labelled queries over the expression types a dashboard sends: a mutation as symbol filter with its coverage, lineages,
    Not / Or / Maybe, True and False."""
    picked = _pick_mutations(data, False, ["main"], per_store=3)[::2]  # "main:<ref><position><symbol>"
    queries = []
    for text in picked:
        position, symbol = int("".join(c for c in text.split(":")[1] if c.isdigit())), text[-1]
        equals = {"type": "NucleotideEquals", "position": position, "symbol": symbol}
        covered = {"type": "Not", "child": {"type": "NucleotideEquals", "position": position, "symbol": "N"}}
        queries.append({"displayLabel": text, "countQuery": equals, "coverageQuery": covered})
        queries.append({"displayLabel": "maybe " + text, "countQuery": {"type": "Maybe", "child": equals}, "coverageQuery": {"type": "True"}})
    aa_position = int("".join(c for c in _pick_mutations(data, True, ["S"], per_store=1)[0].split(":")[1] if c.isdigit()))
    has_aa = {"type": "HasAminoAcidMutation", "sequenceName": "S", "position": aa_position}
    queries += [
        {"displayLabel": "S mutated", "countQuery": has_aa, "coverageQuery": {"type": "True"}},
        {"displayLabel": "B.1.1.7*", "countQuery": LINEAGE, "coverageQuery": {"type": "True"}},
        {"displayLabel": "others", "countQuery": {"type": "Not", "child": LINEAGE}, "coverageQuery": {"type": "Or", "children": [LINEAGE, has_aa]}},
        {"displayLabel": "nothing", "countQuery": {"type": "False"}, "coverageQuery": {"type": "Not", "child": {"type": "True"}}},
        {"displayLabel": "either", "countQuery": {"type": "Or", "children": [has_aa, queries[0]["countQuery"]]}, "coverageQuery": queries[0]["coverageQuery"]},
    ]
    return queries


def test_example_dataset_matches_the_oracle_and_raw_dates(example):
    engine, oracle_db, data = example
    queries = _example_queries(data)
    cache = {}
    seen = []
    for top in TOP_FILTERS:
        for field in ("date", "unsorted_date"):
            action = {"type": "QueriesOverTime", "queries": queries, "dateField": field, "dateRanges": EXAMPLE_RANGES}
            got = engine.execute_query({"action": action, "filterExpression": top})
            assert len(got) == len(queries) * len(EXAMPLE_RANGES)
            assert got == _expected(oracle_db, data, action, top, cache), (top, field)
            seen.append(got)
    assert not any(row["count"] or row["coverage"] for rows in seen[:2] for row in rows)  # the empty top-level filter
    for rows in seen[2:]:  # not vacuous: counts, counts below their coverage, empty cells
        assert any(0 < row["count"] < row["coverage"] for row in rows) and any(row["coverage"] == 0 for row in rows)
        by_label = {row["displayLabel"] for row in rows if row["count"] > 0}
        assert {"S mutated", "B.1.1.7*", "either", queries[0]["displayLabel"]} <= by_label and "nothing" not in by_label
    # both ends are inclusive: a range of one day that rows have counts them
    day = max(set(row["date"] for row in data["rows"] if row.get("date")), key=lambda d: sum(r.get("date") == d for r in data["rows"]))
    action = {"type": "QueriesOverTime", "queries": queries[-4:-3], "dateField": "unsorted_date", "dateRanges": [{"dateFrom": day, "dateTo": day}]}
    got = engine.execute_query({"action": action, "filterExpression": {"type": "True"}})
    assert got == _expected(oracle_db, data, action, {"type": "True"}, cache)
    assert got[0]["coverage"] == sum(row.get("unsorted_date") == day for row in data["rows"]) > 0


def test_equal_sub_expressions_are_counted_once_with_the_same_numbers(example):
    """Two queries with the same coverageQuery text and one whose countQuery is its coverageQuery: the numbers of the same request
    with every sub-expression spelled differently (an And / Or of one child)."""
    engine, _, data = example
    queries = _example_queries(data)
    covered = queries[0]["coverageQuery"]
    shared = [
        {"displayLabel": "a", "countQuery": queries[0]["countQuery"], "coverageQuery": covered},
        {"displayLabel": "b", "countQuery": LINEAGE, "coverageQuery": covered},
        {"displayLabel": "c", "countQuery": covered, "coverageQuery": covered},
        {"displayLabel": "d", "countQuery": LINEAGE, "coverageQuery": LINEAGE},
    ]
    spelled = [
        {"displayLabel": "a", "countQuery": queries[0]["countQuery"], "coverageQuery": covered},
        {"displayLabel": "b", "countQuery": {"type": "And", "children": [LINEAGE]}, "coverageQuery": {"type": "And", "children": [covered]}},
        {"displayLabel": "c", "countQuery": {"type": "Or", "children": [covered]}, "coverageQuery": {"type": "And", "children": [covered, {"type": "True"}]}},
        {"displayLabel": "d", "countQuery": LINEAGE, "coverageQuery": {"type": "Or", "children": [LINEAGE, {"type": "False"}]}},
    ]
    for top in TOP_FILTERS[1:]:
        rows = [engine.execute_query({"action": {"type": "QueriesOverTime", "queries": which, "dateField": "date", "dateRanges": EXAMPLE_RANGES},
                                      "filterExpression": top}) for which in (shared, spelled)]
        assert rows[0] == rows[1]
        c_rows = [row for row in rows[0] if row["displayLabel"] == "c"]
        assert all(row["count"] == row["coverage"] for row in c_rows) and any(row["count"] > 0 for row in c_rows)


def test_more_sub_expressions_than_live_bitsets(example):
    """40 queries with 80 distinct sub-expressions: more than the 64 bitsets the action keeps alive at a time, some of them
    empty or full in a partition (they end a run of filters / go in as all rows)."""
    engine, oracle_db, data = example
    reference = data["nuc_references"]["main"]
    queries = []
    for k in range(40):
        position = 1 + 97 * k % len(reference)
        symbol = reference[position - 1] if k % 3 else "ACGT"[k % 4]
        queries.append({"displayLabel": f"q{k}", "countQuery": {"type": "NucleotideEquals", "position": position, "symbol": symbol},
                        "coverageQuery": {"type": "Not", "child": {"type": "NucleotideEquals", "position": position, "symbol": "N"}}})
    assert len({json.dumps(q[which]) for q in queries for which in ("countQuery", "coverageQuery")}) == 80
    cache = {}
    for top in TOP_FILTERS[1:]:
        action = {"type": "QueriesOverTime", "queries": queries, "dateField": "date", "dateRanges": EXAMPLE_RANGES}
        got = engine.execute_query({"action": action, "filterExpression": top})
        assert got == _expected(oracle_db, data, action, top, cache)
        assert any(row["count"] > 0 for row in got[-5 * 10:]) and any(row["count"] == 0 and row["coverage"] > 0 for row in got)


def test_order_limit_offset(example):
    engine, _, data = example
    queries = _example_queries(data)
    base = {"type": "QueriesOverTime", "queries": queries, "dateField": "date", "dateRanges": EXAMPLE_RANGES}
    rows = engine.execute_query({"action": base, "filterExpression": {"type": "True"}})
    assert len(rows) == len(queries) * len(EXAMPLE_RANGES)
    assert [row["displayLabel"] for row in rows[::len(EXAMPLE_RANGES)]] == [q["displayLabel"] for q in queries]  # queries outermost, request order
    assert [(row["dateFrom"], row["dateTo"]) for row in rows[:len(EXAMPLE_RANGES)]] == [(r["dateFrom"], r["dateTo"]) for r in EXAMPLE_RANGES]
    assert set(rows[0]) == {"displayLabel", "dateFrom", "dateTo", "count", "coverage"}
    in_python = sorted(rows, key=lambda row: (-row["count"], row["displayLabel"]))
    for limit, offset in ((7, 3), (1000, 0), (5, len(rows) - 2)):
        ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "count", "order": "descending"}, "displayLabel"],
                                                       limit=limit, offset=offset), "filterExpression": {"type": "True"}})
        want = in_python[offset:offset + limit]
        # (rows of one label with the same count may come in any order: compared by the ordering's keys, and as a set)
        assert [(row["count"], row["displayLabel"]) for row in ordered] == [(row["count"], row["displayLabel"]) for row in want]
        assert all(row in rows for row in ordered)
    assert len({(row["count"], row["displayLabel"]) for row in in_python[:10]}) > 3
    for field in ("dateFrom", "dateTo", "coverage"):
        assert len(engine.execute_query({"action": dict(base, orderByFields=[field], limit=3), "filterExpression": {"type": "True"}})) == 3
    for field in ("proportion", "mutation", "sequenceName"):
        status, document = engine.execute_raw({"action": dict(base, orderByFields=[field]), "filterExpression": {"type": "True"}})
        assert status == 400 and field in document["message"], document


def _error_cases():
    """(action, what the message has to name)"""
    ranges = [{"dateFrom": "2021-01-01", "dateTo": "2021-01-31"}]
    query = {"displayLabel": "q", "countQuery": LINEAGE, "coverageQuery": {"type": "True"}}
    ok = {"type": "QueriesOverTime", "queries": [query], "dateField": "date", "dateRanges": ranges}

    def without(mapping, key):
        return {k: v for k, v in mapping.items() if k != key}

    return [
        (without(ok, "queries"), "queries"),
        (dict(ok, queries={"displayLabel": "q"}), "queries"),
        (dict(ok, queries=["q"]), "queries"),
        (dict(ok, queries=[without(query, "displayLabel")]), "displayLabel"),
        (dict(ok, queries=[dict(query, displayLabel=3)]), "displayLabel"),
        (dict(ok, queries=[without(query, "countQuery")]), "countQuery"),
        (dict(ok, queries=[dict(query, countQuery="True")]), "countQuery"),
        (dict(ok, queries=[without(query, "coverageQuery")]), "coverageQuery"),
        (dict(ok, queries=[dict(query, coverageQuery=[{"type": "True"}])]), "coverageQuery"),
        (dict(ok, queries=[query, dict(query, countQuery={"type": "True"})]), "displayLabel"),
        (dict(ok, queries=[dict(query, displayLabel=f"q{k}") for k in range(1025)]), "queries"),
        (dict(ok, dateRanges=[{"dateFrom": f"2021-01-{1 + k % 28:02d}", "dateTo": f"2021-01-{1 + k % 28:02d}"} for k in range(1025)]), "date ranges"),
        (dict(ok, dateRanges=[{"dateFrom": "2021-01-01", "dateTo": "2021-01-31"}, {"dateFrom": "2021-01-31", "dateTo": "2021-02-28"}]), "date ranges"),
        (dict(ok, dateRanges=[{"dateFrom": "yesterday", "dateTo": None}]), "dateFrom"),
        (dict(ok, dateRanges=[{"dateFrom": None, "dateTo": "2021-13-45"}]), "dateTo"),
        (dict(ok, dateRanges=[{"dateFrom": "2021-02-01", "dateTo": "2021-01-01"}]), "dateFrom"),
        (without(ok, "dateRanges"), "dateRanges"),
        (without(ok, "dateField"), "dateField"),
        (dict(ok, dateField="region"), "dateField"),
        (dict(ok, dateField="nosuchcolumn"), "dateField"),
        (dict(ok, queries=[dict(query, countQuery={"type": "NoSuchExpression"})]), "countQuery"),
        (dict(ok, queries=[dict(query, coverageQuery={"type": "Not", "child": {"type": "NoSuchExpression"}})]), "coverageQuery"),
    ]


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, data = example
    for action, named in _error_cases():
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 400, (json.dumps(action)[:200], document)
        assert document["error"] == "Bad request"
        assert "QueriesOverTime" in document["message"] and named in document["message"], (named, document)
    # nothing asked for: no rows; the limits themselves are accepted
    ranges = [{"dateFrom": "2021-01-01", "dateTo": "2021-01-31"}]
    query = {"displayLabel": "q", "countQuery": LINEAGE, "coverageQuery": {"type": "True"}}
    for action in ({"type": "QueriesOverTime", "queries": [], "dateField": "date", "dateRanges": ranges},
                   {"type": "QueriesOverTime", "queries": [query], "dateField": "date", "dateRanges": []}):
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 200 and document["queryResult"] == [], document
    day = datetime.date(2020, 1, 1)
    days = [{"dateFrom": str(day + datetime.timedelta(k)), "dateTo": str(day + datetime.timedelta(k))} for k in range(1024)]
    status, document = engine.execute_raw({"action": {"type": "QueriesOverTime", "queries": [query], "dateField": "date", "dateRanges": days},
                                           "filterExpression": {"type": "True"}})
    assert status == 200 and len(document["queryResult"]) == 1024, document
    total = sum(row.get("date") is not None and "2020-01-01" <= row["date"] <= str(day + datetime.timedelta(1023)) for row in data["rows"])
    assert sum(row["coverage"] for row in document["queryResult"]) == total > 0
    many = [dict(query, displayLabel=f"q{k}") for k in range(1024)]
    status, document = engine.execute_raw({"action": {"type": "QueriesOverTime", "queries": many, "dateField": "date", "dateRanges": days[:2]},
                                           "filterExpression": {"type": "True"}})
    assert status == 200 and len(document["queryResult"]) == 2048


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        query = {"displayLabel": "q", "countQuery": LINEAGE, "coverageQuery": {"type": "True"}}
        status, document = engine.execute_raw({"action": {"type": "QueriesOverTime", "queries": [query], "dateField": "date",
                                                          "dateRanges": [{"dateFrom": None, "dateTo": None}]}, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"], document
    finally:
        engine.close()


# ---- a synthetic store that mixes the adaptive layouts, in two partitions ---------------------------------------------------------
SPLIT = 90_001


def _two_partition_engine(sym, days, bucket):
    from silo_amd.engine import Engine

    reference = "".join(NUC_VALID[1 + (p % 4)] for p in range(POSITIONS))
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": reference}], "genes": []})
    engine.set_schema("key", "date")
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    for lo, hi in ((0, SPLIT), (SPLIT, N_ROWS)):
        part = engine.add_partition(hi - lo)
        engine.append_sequences(part, "main", False, 0, [bytes(row).decode() for row in lut[sym[lo:hi]]])
        engine.append_metadata(part, "key", "string", [str(i) for i in range(lo, hi)])
        engine.append_metadata(part, "date", "date", ["" if d < 0 else _day(d) for d in days[lo:hi]])
        engine.append_metadata(part, "row", "int", [str(i) for i in range(lo, hi)])
        engine.append_metadata(part, "bucket", "int", [str(b) for b in bucket[lo:hi]])
    engine.finalize()
    return engine


def test_adaptive_layouts_match_numpy(built):
    """140 003 rows in two partitions, the store in its default layout with positions of every kind (even positions: one symbol
    derived; odd ones: one-hot rows; position 5: code planes): symbol filters there as countQuery, 'not N' as coverageQuery,
    against numpy on the raw symbol matrix and dates."""
    from silo_amd import binding

    rng = np.random.default_rng(2024)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    lib = binding.load_library()
    lib.silo_gpu_tune(9, -1)  # no charge per kind of launch: with it a store this short would never mix layouts
    try:
        engine = _two_partition_engine(sym, days, bucket)
    finally:
        lib.silo_gpu_tune(9, 0)
    try:
        cells = []
        for p in (0, 2, 1, 3, 5, 46, 47):
            column = sym[:, p]
            counts = np.bincount(column[column <= 4], minlength=5)
            for s in np.argsort(-counts, kind="stable")[:2].tolist() + [int(rng.integers(5, 15))]:  # the two commonest, an ambiguity code
                cells.append((p, s))
        queries = [{"displayLabel": f"{p + 1}{NUC_CHARS[s]}", "countQuery": {"type": "NucleotideEquals", "position": p + 1, "symbol": NUC_CHARS[s]},
                    "coverageQuery": {"type": "Not", "child": {"type": "NucleotideEquals", "position": p + 1, "symbol": "N"}}} for p, s in cells]
        rows = np.arange(N_ROWS)
        tops = [
            ({"type": "True"}, np.ones(N_ROWS, dtype=bool)),
            ({"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7),
            ({"type": "IntBetween", "column": "row", "from": 60_000, "to": 101_000}, (rows >= 60_000) & (rows <= 101_000)),  # across the partitions
            ({"type": "IntBetween", "column": "row", "from": SPLIT, "to": None}, rows >= SPLIT),                             # none of the first, all of the second
        ]
        for expression, selected in tops:
            action = {"type": "QueriesOverTime", "queries": queries, "dateField": "date",
                      "dateRanges": [_range_json(low, high) for low, high in SYNTHETIC_RANGES]}
            got = engine.execute_query({"action": action, "filterExpression": expression})
            assert len(got) == len(cells) * len(SYNTHETIC_RANGES)
            k = 0
            for p, s in cells:
                for low, high in SYNTHETIC_RANGES:
                    in_range = selected & (days >= (0 if low is None else low)) & (days <= (10 ** 6 if high is None else high))
                    want = (int(np.count_nonzero(in_range & (sym[:, p] == s))), int(np.count_nonzero(in_range & (sym[:, p] != 15))))
                    assert (got[k]["count"], got[k]["coverage"]) == want, (expression, p, s, low, high)
                    k += 1
            assert any(r["count"] > 0 for r in got) and any(r["coverage"] == 0 for r in got)
    finally:
        engine.close()
