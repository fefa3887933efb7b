"""CrossTabulation: per (row query, column query) the rows of the filter that match both, with the marginals and the total, from
the pair count kernel (K9), through JSON and the engine: against row sets the oracle selects for And(filter, sub-expression)
intersected on the host, against Aggregated under And(filter, row, column), and on a synthetic store that mixes the adaptive
layouts against numpy on the raw symbol matrix."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.cross_filters_reference import cross_filter_counts  # noqa: E402
from tests.test_mutations_over_time_gpu import (  # noqa: E402
    N_ROWS, NUC_CHARS, _build_example_engine, _pick_mutations, _synthetic_dates, _synthetic_matrix)
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE, SPLIT, TOP_FILTERS, _two_partition_engine  # noqa: E402

FIELDS = {"rowLabel", "columnLabel", "count", "rowCount", "columnCount", "total"}


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


def _expected(oracle_db, action, top, cache):
    """Every row of the response from the row sets the oracle selects for And(top, sub-expression), intersected here."""
    total = _selected_keys(oracle_db, top, cache)
    rows = action["rowQueries"]
    columns = action.get("columnQueries", rows)
    row_sets = [_selected_keys(oracle_db, {"type": "And", "children": [top, entry["query"]]}, cache) for entry in rows]
    column_sets = [_selected_keys(oracle_db, {"type": "And", "children": [top, entry["query"]]}, cache) for entry in columns]
    return [{"rowLabel": row["displayLabel"], "columnLabel": column["displayLabel"], "count": len(row_set & column_set),
             "rowCount": len(row_set), "columnCount": len(column_set), "total": len(total)}
            for row, row_set in zip(rows, row_sets) for column, column_set in zip(columns, column_sets)]


def _run(engine, action, top):
    return engine.execute_query({"action": dict(action, type="CrossTabulation"), "filterExpression": top})


def _example_lists(data):
    """Row queries: mutations as symbol filters, a Maybe, an Or, True and False; column queries: lineages, a Not, an amino acid
    mutation, and the first row query again (equal text on both sides)."""
    rows = []
    for text in _pick_mutations(data, False, ["main"], per_store=3)[::2]:  # "main:<ref><position><symbol>"
        position, symbol = int("".join(c for c in text.split(":")[1] if c.isdigit())), text[-1]
        equals = {"type": "NucleotideEquals", "position": position, "symbol": symbol}
        rows.append({"displayLabel": text, "query": equals})
        rows.append({"displayLabel": "maybe " + text, "query": {"type": "Maybe", "child": equals}})
    aa_position = int("".join(c for c in _pick_mutations(data, True, ["S"], per_store=1)[0].split(":")[1] if c.isdigit()))
    has_aa = {"type": "HasAminoAcidMutation", "sequenceName": "S", "position": aa_position}
    rows += [
        {"displayLabel": "either", "query": {"type": "Or", "children": [has_aa, rows[0]["query"]]}},
        {"displayLabel": "everything", "query": {"type": "True"}},
        {"displayLabel": "nothing", "query": {"type": "False"}},
    ]
    columns = [
        {"displayLabel": "B.1.1.7*", "query": LINEAGE},
        {"displayLabel": "others", "query": {"type": "Not", "child": LINEAGE}},
        {"displayLabel": "S mutated", "query": has_aa},
        {"displayLabel": "again", "query": rows[0]["query"]},
        {"displayLabel": "Switzerland", "query": {"type": "StringEquals", "column": "country", "value": "Switzerland"}},
    ]
    return rows, columns


def test_example_dataset_matches_the_oracle(example):
    engine, oracle_db, data = example
    rows, columns = _example_lists(data)
    cache = {}
    seen = []
    for top in TOP_FILTERS:  # selects nothing, a lineage, everything
        action = {"rowQueries": rows, "columnQueries": columns}
        got = _run(engine, action, top)
        assert len(got) == len(rows) * len(columns) and all(set(row) == FIELDS for row in got)
        assert got == _expected(oracle_db, action, top, cache), top
        seen.append(got)
    assert not any(row[field] for row in seen[0] for field in ("count", "rowCount", "columnCount", "total"))  # the empty filter
    assert all(row["total"] == len(data["rows"]) for row in seen[2])                                             # the full one
    assert any(row["count"] == 0 and row["rowCount"] > 0 and row["columnLabel"] == "others" for row in seen[1])  # disjoint under the lineage
    for got in seen[1:]:  # not vacuous: cells below both marginals
        assert any(0 < row["count"] < min(row["rowCount"], row["columnCount"]) for row in got)
        by_row = {row["rowLabel"]: row for row in got if row["columnLabel"] == "again"}
        assert by_row[rows[0]["displayLabel"]]["count"] == by_row[rows[0]["displayLabel"]]["rowCount"] > 0  # equal text on both sides
        assert by_row["everything"]["rowCount"] == by_row["everything"]["total"] and by_row["nothing"]["rowCount"] == 0


def test_no_column_queries_gives_the_symmetric_matrix(example):
    engine, oracle_db, data = example
    rows, columns = _example_lists(data)
    entries = rows[:4] + columns[:3]
    cache = {}
    for top in TOP_FILTERS[1:]:
        got = _run(engine, {"rowQueries": entries}, top)
        assert got == _expected(oracle_db, {"rowQueries": entries}, top, cache)
        assert got == _run(engine, {"rowQueries": entries, "columnQueries": entries}, top)
        cells = {(row["rowLabel"], row["columnLabel"]): row for row in got}
        for (a, b), row in cells.items():
            assert row["count"] == cells[b, a]["count"] and row["rowCount"] == cells[b, a]["columnCount"]
            if a == b:
                assert row["count"] == row["rowCount"] == row["columnCount"]
        assert any(row["count"] > 0 for (a, b), row in cells.items() if a != b)


def test_more_sub_expressions_than_a_batch_on_either_side(example):
    """40 x 35 distinct sub-expressions: more per side than half the bitsets the action keeps alive, so both batch loops turn over;
    some are empty or full in a partition (left out of a call / passed as all rows)."""
    engine, oracle_db, data = example
    reference = data["nuc_references"]["main"]

    def entry(label, k, step):
        position = 1 + step * k % len(reference)
        symbol = reference[position - 1] if k % 3 else "ACGT"[k % 4]
        return {"displayLabel": f"{label}{k}", "query": {"type": "NucleotideEquals", "position": position, "symbol": symbol}}

    rows = [entry("r", k, 97) for k in range(40)]
    columns = [entry("c", k, 89) for k in range(1, 36)]
    assert len({json.dumps(e["query"]) for e in rows}) == 40 and len({json.dumps(e["query"]) for e in columns}) == 35
    cache = {}
    for top in TOP_FILTERS[1:]:
        action = {"rowQueries": rows, "columnQueries": columns}
        got = _run(engine, action, top)
        assert got == _expected(oracle_db, action, top, cache)
        assert any(row["count"] > 0 for row in got[-35 * 5:]) and any(row["count"] > 0 for row in got if row["columnLabel"] in ("c34", "c35"))
        assert any(row["count"] == 0 and row["columnCount"] > 0 for row in got)
        assert any(0 < row["count"] < min(row["rowCount"], row["columnCount"]) for row in got)


def test_a_sub_expression_empty_in_one_partition_and_full_in_another(example):
    """The key of row 37 — the only row of the second of three partitions: all of that partition, nothing of the others."""
    engine, oracle_db, data = example
    key = data["rows"][37]["gisaid_epi_isl"]
    one_row = {"displayLabel": "row 37", "query": {"type": "StringEquals", "column": "gisaid_epi_isl", "value": key}}
    rows, columns = _example_lists(data)
    cache = {}
    for action in ({"rowQueries": [one_row] + rows[:3], "columnQueries": columns + [one_row]}, {"rowQueries": [one_row, rows[0], columns[1]]}):
        got = _run(engine, action, {"type": "True"})
        assert got == _expected(oracle_db, action, {"type": "True"}, cache)
        assert [row["count"] for row in got if row["rowLabel"] == row["columnLabel"] == "row 37"] == [1]
        assert sum(row["count"] for row in got if row["rowLabel"] == "row 37") >= 2


def test_cells_agree_with_aggregated(example):
    engine, _, data = example
    rows, columns = _example_lists(data)
    top = TOP_FILTERS[1]
    got = {(row["rowLabel"], row["columnLabel"]): row for row in _run(engine, {"rowQueries": rows, "columnQueries": columns}, top)}

    def aggregated(*expressions):
        return engine.execute_query({"action": {"type": "Aggregated"}, "filterExpression": {"type": "And", "children": [top, *expressions]}})[0]["count"]

    for row, column in ((rows[0], columns[0]), (rows[1], columns[2]), (rows[-3], columns[1]), (rows[-2], columns[3]), (rows[-1], columns[0])):
        cell = got[row["displayLabel"], column["displayLabel"]]
        assert cell["count"] == aggregated(row["query"], column["query"])
        assert cell["rowCount"] == aggregated(row["query"]) and cell["columnCount"] == aggregated(column["query"]) and cell["total"] == aggregated()
    assert got[rows[0]["displayLabel"], columns[0]["displayLabel"]]["count"] > 0


def test_order_limit_offset(example):
    engine, _, data = example
    rows, columns = _example_lists(data)
    base = {"type": "CrossTabulation", "rowQueries": rows, "columnQueries": columns}
    everything = {"type": "True"}
    got = engine.execute_query({"action": base, "filterExpression": everything})
    # row queries outermost, both in request order
    assert [row["rowLabel"] for row in got[::len(columns)]] == [entry["displayLabel"] for entry in rows]
    assert [row["columnLabel"] for row in got[:len(columns)]] == [entry["displayLabel"] for entry in columns]
    in_python = sorted(got, key=lambda row: (-row["count"], row["rowLabel"], row["columnLabel"]))
    for limit, offset in ((7, 3), (1000, 0), (5, len(got) - 2)):
        ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "count", "order": "descending"}, "rowLabel", "columnLabel"],
                                                       limit=limit, offset=offset), "filterExpression": everything})
        assert ordered == in_python[offset:offset + limit]
    assert len({row["count"] for row in in_python[:10]}) > 2
    for field in ("rowCount", "columnCount", "total"):
        assert len(engine.execute_query({"action": dict(base, orderByFields=[field], limit=3), "filterExpression": everything})) == 3
    for field in ("displayLabel", "coverage", "proportion"):
        status, document = engine.execute_raw({"action": dict(base, orderByFields=[field]), "filterExpression": everything})
        assert status == 400 and field in document["message"], document


def _error_cases():
    """(action, what the message has to name)"""
    entry = {"displayLabel": "q", "query": LINEAGE}
    ok = {"type": "CrossTabulation", "rowQueries": [entry], "columnQueries": [entry]}

    def without(mapping, key):
        return {k: v for k, v in mapping.items() if k != key}

    def many(count):
        return [dict(entry, displayLabel=f"q{k}") for k in range(count)]

    return [
        (without(ok, "rowQueries"), "rowQueries"),
        (dict(ok, rowQueries={"displayLabel": "q"}), "rowQueries"),
        (dict(ok, columnQueries="q"), "columnQueries"),
        (dict(ok, columnQueries=None), "columnQueries"),
        (dict(ok, rowQueries=["q"]), "rowQueries"),
        (dict(ok, columnQueries=[entry, 3]), "columnQueries"),
        (dict(ok, rowQueries=[without(entry, "displayLabel")]), "displayLabel"),
        (dict(ok, columnQueries=[dict(entry, displayLabel=3)]), "displayLabel"),
        (dict(ok, rowQueries=[without(entry, "query")]), "query"),
        (dict(ok, columnQueries=[dict(entry, query="True")]), "query"),
        (dict(ok, rowQueries=[dict(entry, query=[{"type": "True"}])]), "query"),
        (dict(ok, rowQueries=[entry, dict(entry, query={"type": "True"})]), "displayLabel"),
        (dict(ok, columnQueries=[entry, dict(entry, query={"type": "True"})]), "displayLabel"),
        (dict(ok, rowQueries=[dict(entry, query={"type": "NoSuchExpression"})]), "query"),
        (dict(ok, columnQueries=[dict(entry, query={"type": "Not", "child": {"type": "NoSuchExpression"}})]), "query"),
        (dict(ok, rowQueries=many(1025)), "rowQueries"),
        (dict(ok, columnQueries=many(1025)), "columnQueries"),
        (dict(ok, rowQueries=many(257), columnQueries=many(256)), "cells"),
        (dict(without(ok, "columnQueries"), rowQueries=many(257)), "cells"),
    ]


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, data = example
    for action, named in _error_cases():
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 400, (json.dumps(action)[:200], document)
        assert document["error"] == "Bad request"
        assert "CrossTabulation" in document["message"] and named in document["message"], (named, document)
    # the same label in both lists is fine; nothing asked for: no rows; the limits themselves are accepted
    entry = {"displayLabel": "q", "query": LINEAGE}
    status, document = engine.execute_raw({"action": {"type": "CrossTabulation", "rowQueries": [entry], "columnQueries": [entry]},
                                           "filterExpression": {"type": "True"}})
    assert status == 200 and len(document["queryResult"]) == 1 and document["queryResult"][0]["count"] == document["queryResult"][0]["rowCount"] > 0
    for action in ({"type": "CrossTabulation", "rowQueries": []}, {"type": "CrossTabulation", "rowQueries": [], "columnQueries": [entry]},
                   {"type": "CrossTabulation", "rowQueries": [entry], "columnQueries": []}):
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 200 and document["queryResult"] == [], document
    reference = data["nuc_references"]["main"]
    many = [{"displayLabel": f"q{k}", "query": {"type": "NucleotideEquals", "position": k + 1, "symbol": reference[k]}} for k in range(1024)]
    for action in ({"type": "CrossTabulation", "rowQueries": many, "columnQueries": many[:64]},
                   {"type": "CrossTabulation", "rowQueries": many[:2], "columnQueries": many}):
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 200 and len(document["queryResult"]) == len(action["rowQueries"]) * len(action["columnQueries"]), document
        assert all(row["count"] <= row["rowCount"] <= row["total"] == len(data["rows"]) for row in document["queryResult"])
        assert any(row["count"] > 0 for row in document["queryResult"][-64:])


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        entry = {"displayLabel": "q", "query": LINEAGE}
        status, document = engine.execute_raw({"action": {"type": "CrossTabulation", "rowQueries": [entry]}, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"] and "CrossTabulation" in document["message"], document
    finally:
        engine.close()


# ---- a synthetic store that mixes the adaptive layouts, in two partitions ---------------------------------------------------------
def test_adaptive_layouts_match_numpy(built):
    """140 003 rows in two partitions, the store in its default layout with positions of every kind (even positions: one symbol
    derived; odd ones: one-hot rows; position 5: code planes): symbol filters there on both sides, against numpy on the raw symbol
    matrix."""
    from silo_amd import binding

    rng = np.random.default_rng(2025)
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
        def cells_at(positions):
            cells = []
            for p in positions:
                column = sym[:, p]
                counts = np.bincount(column[column <= 4], minlength=5)
                for s in np.argsort(-counts, kind="stable")[:2].tolist() + [int(rng.integers(5, 15))]:  # the two commonest, an ambiguity code
                    cells.append((p, s))
            return cells

        def entries(cells):
            return [{"displayLabel": f"{p + 1}{NUC_CHARS[s]}", "query": {"type": "NucleotideEquals", "position": p + 1, "symbol": NUC_CHARS[s]}} for p, s in cells]

        row_cells, column_cells = cells_at((0, 2, 1, 3, 5)), cells_at((5, 46, 47, 4))
        action = {"rowQueries": entries(row_cells), "columnQueries": entries(column_cells)}
        row_masks = [sym[:, p] == s for p, s in row_cells]
        column_masks = [sym[:, p] == s for p, s in column_cells]
        rows = np.arange(N_ROWS)
        tops = [
            ({"type": "True"}, np.ones(N_ROWS, dtype=bool)),
            ({"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7),
            ({"type": "IntBetween", "column": "row", "from": 60_000, "to": 101_000}, (rows >= 60_000) & (rows <= 101_000)),  # across the partitions
            ({"type": "IntBetween", "column": "row", "from": SPLIT, "to": None}, rows >= SPLIT),                             # none of the first, all of the second
        ]
        for expression, selected in tops:
            got = _run(engine, action, expression)
            want = cross_filter_counts(selected, row_masks + [None], column_masks + [None], N_ROWS)
            assert len(got) == len(row_cells) * len(column_cells)
            k = 0
            for i in range(len(row_cells)):
                for j in range(len(column_cells)):
                    numbers = (got[k]["count"], got[k]["rowCount"], got[k]["columnCount"], got[k]["total"])
                    assert numbers == (int(want[i, j]), int(want[i, -1]), int(want[-1, j]), int(want[-1, -1])), (expression, row_cells[i], column_cells[j])
                    k += 1
            assert any(r["count"] > 0 for r in got) and any(r["count"] == 0 for r in got)
    finally:
        engine.close()
