#!/usr/bin/env python3
"""QueriesOverTime probe: 20 labelled queries x 52 weekly ranges in ONE request against the same cells as 2 x 20 x 52 Aggregated
requests (And(filter, countQuery or coverageQuery, DateBetween(date, week))), on bench.py's 10 M-row synthetic database with a
date column appended (rows in (lineage, date) order within the store's row order, as a sorted store has them).  Each timing is a
host clock around requests that end in a device -> host fetch the host waits for; medians of --reps runs, the two forms
alternated.  Prints one JSON line; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd"), os.path.join(ROOT, "tools")]

import bench  # noqa: E402
from mutations_over_time_probe import EPOCH, _runs  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--queries", type=int, default=20)
    parser.add_argument("--weeks", type=int, default=52)
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    texts = [str(EPOCH + datetime.timedelta(int(d))) for d in range(7 * args.weeks + 1)]

    def add_dates(engine, partition, n_sequences):
        # as tools/mutations_over_time_probe.py: a random day per row, the rows of each lineage in date order
        from silo_amd import synth

        lineage = synth.assign_lineages(n_sequences, synth.make_lineage_tree(bench.N_LINEAGES), synth.DEFAULT_SEED)
        days = np.random.default_rng(7).integers(0, 7 * args.weeks, size=n_sequences)
        order = np.argsort(lineage, kind="stable")
        dated = np.empty(n_sequences, dtype=np.int64)
        for start, end in _runs(lineage[order]):
            dated[order[start:end]] = np.sort(days[order[start:end]])
        engine.append_metadata(partition, "date", "date", [texts[d] for d in dated])

    t0 = time.perf_counter()
    bench.add_synthetic_metadata = add_dates
    engine, _, _, _, _ = bench.build_engine(args.sequences, 0, 1, None, 0, with_metadata=True)
    build_s = time.perf_counter() - t0

    reference = bench.load_reference_genomes()["nucleotideSequences"][0]["sequence"]
    positions = np.linspace(100, len(reference) - 100, args.queries).astype(int)
    # a mutation as a dashboard asks for it: the rows that carry the symbol, over the rows that have any symbol but N there
    queries = [{"displayLabel": f"{reference[p]}{p + 1}{'T' if reference[p] != 'T' else 'C'}",
                "countQuery": {"type": "NucleotideEquals", "position": int(p) + 1, "symbol": "T" if reference[p] != "T" else "C"},
                "coverageQuery": {"type": "Not", "child": {"type": "NucleotideEquals", "position": int(p) + 1, "symbol": "N"}}} for p in positions]
    ranges = [{"dateFrom": texts[7 * w], "dateTo": texts[7 * w + 6]} for w in range(args.weeks)]
    lineage_filter = {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}
    grouped = json.dumps({"action": {"type": "QueriesOverTime", "queries": queries, "dateField": "date", "dateRanges": ranges},
                          "filterExpression": lineage_filter}).encode()
    # "date" is not the dateToSortBy column here: DateBetween's upper bound is exclusive on it, so the week ends at the next day
    single = [json.dumps({"action": {"type": "Aggregated"},
                          "filterExpression": {"type": "And", "children": [
                              lineage_filter, query[which], {"type": "DateBetween", "column": "date", "from": texts[7 * w], "to": texts[7 * w + 7]}]}}).encode()
              for query in queries for w in range(args.weeks) for which in ("countQuery", "coverageQuery")]

    def run_grouped():
        status, body = engine.execute_text(grouped)
        assert status == 200, body[:500]
        return json.loads(body.decode())["queryResult"]

    def run_single():
        out = []
        for query in single:
            status, body = engine.execute_text(query)
            assert status == 200, body[:500]
            out.append(json.loads(body.decode())["queryResult"][0]["count"])
        return out

    rows = run_grouped()
    counts = run_single()
    assert [value for row in rows for value in (row["count"], row["coverage"])] == counts  # the two forms agree on every cell
    grouped_ms, single_ms = [], []
    for _ in range(args.reps):  # alternated, so that drift hits both
        t = time.perf_counter()
        run_grouped()
        grouped_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        run_single()
        single_ms.append((time.perf_counter() - t) * 1e3)
    print(json.dumps({
        "sequences": args.sequences, "queries": args.queries, "weeks": args.weeks, "build_s": round(build_s, 1),
        "queries_over_time_ms": [round(x, 3) for x in grouped_ms], "aggregated_requests": len(single),
        "aggregated_ms": [round(x, 3) for x in single_ms],
        "queries_over_time_ms_median": round(float(np.median(grouped_ms)), 3), "aggregated_ms_median": round(float(np.median(single_ms)), 3),
        "cells_with_count": sum(1 for r in rows if r["count"] > 0),
    }), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
