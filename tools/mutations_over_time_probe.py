#!/usr/bin/env python3
"""MutationsOverTime probe: 100 mutations x 52 weekly ranges in ONE query against the 52 equivalent Mutations queries
(And(PangoLineage B.1*, DateBetween(date, week))), on bench.py's 10 M-row synthetic database with a date column appended
(rows in (lineage, date) order within the store's row order, as a sorted store has them).  Each timing is a host clock around
queries that end in a device -> host fetch the host waits for.  Prints one JSON line; run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd")]

import bench  # noqa: E402

EPOCH = datetime.date(2021, 1, 4)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--mutations", type=int, default=100)
    parser.add_argument("--weeks", type=int, default=52)
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    texts = [str(EPOCH + datetime.timedelta(int(d))) for d in range(7 * args.weeks + 1)]

    def add_dates(engine, partition, n_sequences):
        # the date column, in place of bench.py's synthetic metadata: a random week day per row, the rows of each lineage in
        # date order (the store's (lineage, date, key) order within the lineage's rows)
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
    positions = np.linspace(100, len(reference) - 100, args.mutations).astype(int)
    mutations = [f"{reference[p]}{p + 1}{'T' if reference[p] != 'T' else 'C'}" for p in positions]
    ranges = [{"dateFrom": texts[7 * w], "dateTo": texts[7 * w + 6]} for w in range(args.weeks)]
    lineage_filter = {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}
    grouped = json.dumps({"action": {"type": "MutationsOverTime", "mutations": mutations, "dateField": "date", "dateRanges": ranges},
                          "filterExpression": lineage_filter}).encode()
    # "date" is not the dateToSortBy column here: DateBetween's upper bound is exclusive on it, so the week ends at the next day
    per_week = [json.dumps({"action": {"type": "Mutations", "minProportion": 0},
                            "filterExpression": {"type": "And", "children": [
                                lineage_filter, {"type": "DateBetween", "column": "date", "from": texts[7 * w], "to": texts[7 * w + 7]}]}}).encode()
                for w in range(args.weeks)]

    def run_grouped():
        status, body = engine.execute_text(grouped)
        assert status == 200, body[:500]
        return json.loads(body.decode())["queryResult"]

    def run_weeks():
        out = []
        for query in per_week:
            status, body = engine.execute_text(query)
            assert status == 200, body[:500]
            out.append(json.loads(body.decode())["queryResult"])
        return out

    rows = run_grouped()
    weeks = run_weeks()
    # the two agree on every cell the Mutations queries report
    for m, name in enumerate(mutations):
        for w in range(args.weeks):
            row = rows[m * args.weeks + w]
            other = {r["mutation"]: r for r in weeks[w]}.get(name)
            assert (other["count"] if other else 0) == row["count"], (name, w, other, row)
    grouped_ms, weeks_ms = [], []
    for _ in range(args.reps):  # alternated, so that drift hits both
        t = time.perf_counter()
        run_grouped()
        grouped_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        run_weeks()
        weeks_ms.append((time.perf_counter() - t) * 1e3)
    print(json.dumps({
        "sequences": args.sequences, "mutations": args.mutations, "weeks": args.weeks, "build_s": round(build_s, 1),
        "grouped_ms": [round(x, 3) for x in grouped_ms], "weekly_mutations_ms": [round(x, 3) for x in weeks_ms],
        "grouped_ms_median": round(float(np.median(grouped_ms)), 3), "weekly_mutations_ms_median": round(float(np.median(weeks_ms)), 3),
        "cells_with_count": sum(1 for r in rows if r["count"] > 0),
    }), flush=True)
    engine.close()


def _runs(values):
    """[start, end) of the runs of equal values."""
    edges = np.flatnonzero(np.diff(values)) + 1
    starts = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [len(values)]])
    return zip(starts.tolist(), ends.tolist())


if __name__ == "__main__":
    main()
