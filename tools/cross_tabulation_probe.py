#!/usr/bin/env python3
"""CrossTabulation probe: N x N symbol filters in ONE request against the same cells as Aggregated requests
(And(filter, row, column)) through silo_engine_execute_batch, on bench.py's 10 M-row synthetic database under a PangoLineage
filter.  --pairs 0 sends every pair as an Aggregated request; --pairs K sends a sample of K pairs (every (N * N / K)-th cell in
row-major order) and reports the time scaled to all N * N.  Each timing is a host clock around requests that end in a
device -> host fetch the host waits for; medians of --reps runs, the two forms alternated.  Prints one JSON line per --side;
run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split (k_cross_filter_counts, the filter kernels)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd"), os.path.join(ROOT, "tools")]

import bench  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--side", type=int, nargs="+", default=[64, 256], help="filters per side; one measurement each")
    parser.add_argument("--pairs", type=int, default=4096, help="Aggregated requests sent at most per side (0 = every pair)")
    parser.add_argument("--batch", type=int, default=256, help="Aggregated requests per silo_engine_execute_batch call")
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--skip-aggregated", action="store_true", help="only the CrossTabulation request (for a profiler run)")
    args = parser.parse_args()

    t0 = time.perf_counter()
    engine, _, _, _, _ = bench.build_engine(args.sequences, 0, 1, None, 0)
    build_s = time.perf_counter() - t0

    reference = bench.load_reference_genomes()["nucleotideSequences"][0]["sequence"]
    lineage_filter = {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}
    for side in args.side:
        # rows: a mutation per position; columns: the reference symbol at other positions
        row_positions = np.linspace(100, len(reference) - 200, side).astype(int)
        rows = [{"displayLabel": f"r{p + 1}", "query": {"type": "NucleotideEquals", "position": int(p) + 1, "symbol": "T" if reference[p] != "T" else "C"}}
                for p in row_positions]
        columns = [{"displayLabel": f"c{p + 51}", "query": {"type": "NucleotideEquals", "position": int(p) + 51, "symbol": reference[p + 50]}}
                   for p in row_positions]
        cross = json.dumps({"action": {"type": "CrossTabulation", "rowQueries": rows, "columnQueries": columns}, "filterExpression": lineage_filter}).encode()
        cells = side * side
        stride = 1 if args.pairs == 0 else max(1, cells // args.pairs)
        sample = list(range(0, cells, stride))
        single = [json.dumps({"action": {"type": "Aggregated"},
                              "filterExpression": {"type": "And", "children": [lineage_filter, rows[k // side]["query"], columns[k % side]["query"]]}}).encode()
                  for k in sample]

        def run_cross():
            status, body = engine.execute_text(cross)
            assert status == 200, body[:500]
            return json.loads(body.decode())["queryResult"]

        def run_single():
            out = []
            for begin in range(0, len(single), args.batch):
                for status, body in engine.execute_batch_text(single[begin:begin + args.batch]):
                    assert status == 200, body[:500]
                    out.append(json.loads(body.decode())["queryResult"][0]["count"])
            return out

        table = run_cross()
        result = {"sequences": args.sequences, "side": side, "cells": cells, "build_s": round(build_s, 1), "total": table[0]["total"],
                  "cells_with_count": sum(1 for r in table if r["count"] > 0)}
        cross_ms, single_ms = [], []
        if not args.skip_aggregated:
            assert [table[k]["count"] for k in sample] == run_single()  # the two forms agree on every sampled cell
        for _ in range(args.reps):  # alternated, so that drift hits both
            t = time.perf_counter()
            run_cross()
            cross_ms.append((time.perf_counter() - t) * 1e3)
            if not args.skip_aggregated:
                t = time.perf_counter()
                run_single()
                single_ms.append((time.perf_counter() - t) * 1e3)
        result.update(cross_tabulation_ms=[round(x, 3) for x in cross_ms], cross_tabulation_ms_median=round(float(np.median(cross_ms)), 3))
        if single_ms:
            median = float(np.median(single_ms))
            result.update(aggregated_requests=len(single), aggregated_batch=args.batch, aggregated_ms=[round(x, 3) for x in single_ms],
                          aggregated_ms_median=round(median, 3), aggregated_ms_scaled_to_all_cells=round(median * cells / len(single), 3))
        print(json.dumps(result), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
