#!/usr/bin/env python3
"""Region cell-count probe (K23): bench.py's synthetic genome store (--sequences rows, one partition) built through the binding.  HIP
events on the null stream, median of --reps runs behind one warm-up each:
  - silo_gpu_region_cell_values as a whole (its table upload, the plane pass and the key, run and sparse passes behind it on one
    stream) for one region of 1, 24 and 3 822 positions and for the whole sequence, and for 98 tiling regions of 400 positions
    whose neighbours overlap (by at least 30 positions), in their two colour classes; beside each, in the same run, silo_gpu_row_cell_counts (K22's
    whole-sequence build) and silo_gpu_stream_read_probe over the plane bytes of the positions the call walks plus the columns it
    writes;
  - silo_gpu_bitset_from_values and silo_gpu_count_values (1 and 49 columns; all rows and bench.py's lineage filter) on the columns
    those calls left, against silo_gpu_stream_read_probe over the bytes each must read.
--engine instead times requests through the engine on the same store: `Aggregated` under a spike-coverage CellCount (missing in
21 563 .. 25 384 at most 0) and a 98-region CellCountByRegion under bench.py's lineage filter.
Prints one JSON line per case; no ratio is asserted."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd"), os.path.join(ROOT, "tools")]

import bench  # noqa: E402
from distinct_probe import synthetic_model, words_of  # noqa: E402

SPIKE = (21563, 25384)  # 1-based inclusive: 3 822 positions


def tiling(positions, length=400, overlap=30, count=98):
    """`count` regions [first, end) of `length` positions spread evenly over the sequence: neighbours overlap by at least `overlap`
    positions (98 regions of 400 over 29 903 positions: by 96) and a region meets no other than its neighbours — two colour classes."""
    step = (positions - length) // (count - 1)
    assert length - step >= overlap and 2 * step >= length
    return [(k * step, k * step + length) for k in range(count)]


def colour(ranges):
    """The chunks of CellCountByRegion (host/sequence_actions.cpp): by start, the first chunk where the region overlaps none."""
    chunks = []
    for region in sorted(range(len(ranges)), key=lambda g: ranges[g][0]):
        for chunk in chunks:
            if ranges[chunk[-1]][1] <= ranges[region][0]:
                chunk.append(region)
                break
        else:
            chunks.append([region])
    return chunks


def through_the_engine(args):
    """--engine: the host clock around whole requests, one JSON line."""
    from silo_amd.engine import Engine

    n = args.sequences
    genomes, _, tree, lineage, model = synthetic_model(n)
    positions = len(genomes["nucleotideSequences"][0]["sequence"])
    engine = Engine(genomes)
    engine.set_schema("key", None)
    partition = engine.add_partition(n)
    engine.generate_synthetic(partition, "main", False, model, engine.position_window("main", False))
    engine.set_lineage_column_ids(partition, "pango_lineage", tree.names, lineage)
    engine.append_metadata(partition, "key", "string", [f"S{i}" for i in range(n)])
    engine.finalize()

    def request_ms(request):
        text = json.dumps(request).encode()
        times = []
        for _ in range(args.reps + 1):
            t = time.perf_counter()
            status, body = engine.execute_text(text)
            times.append((time.perf_counter() - t) * 1e3)
            assert status == 200, body[:500]
        return round(float(np.median(times[1:])), 4), json.loads(body.decode())["queryResult"]

    coverage = {"type": "CellCount", "cells": "missing", "positionFrom": SPIKE[0], "positionTo": SPIKE[1], "atMost": 0}
    coverage_ms, coverage_rows = request_ms({"action": {"type": "Aggregated"}, "filterExpression": coverage})
    lineage_filter = {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}
    regions = [{"name": f"amplicon {k}", "positionFrom": first + 1, "positionTo": end, "atLeast": (end - first) // 2} for k, (first, end) in enumerate(tiling(positions))]
    table_ms, table = request_ms({"action": {"type": "CellCountByRegion", "cells": "missing", "regions": regions}, "filterExpression": lineage_filter})
    print(json.dumps({
        "sequences": n, "positions": positions, "aggregated_under_spike_coverage_ms": coverage_ms, "spike_coverage_rows": coverage_rows[0]["count"],
        "cell_count_by_region_98_under_lineage_ms": table_ms, "lineage_rows": table[0]["total"], "regions_with_dropouts": sum(1 for row in table if row["count"]),
    }), flush=True)
    engine.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--build-reps", type=int, default=5)
    parser.add_argument("--engine", action="store_true", help="time requests through the engine instead of the C entries")
    args = parser.parse_args()
    if args.engine:
        return through_the_engine(args)

    from silo_amd import binding

    lib = binding.load_library()
    n = args.sequences
    _, reference, tree, lineage, model = synthetic_model(n)
    member = tree.subtree(tree.names.index(bench.QUERY_LINEAGE)).astype(bool)

    def timed(launches, reps):
        """Median of HIP event timings (ms) around `launches`, behind one warm-up run."""
        times = []
        for _ in range(reps + 1):
            events = [binding.GpuEvent() for _ in range(2)]
            events[0].record()
            launches()
            events[1].record()
            binding._check(lib.silo_gpu_stream_synchronize(None))
            times.append(events[0].elapsed_ms(events[1]))
        return round(float(np.median(times[1:])), 4)

    def stream_read_ms(nbytes):
        read_ms = ctypes.c_float()
        binding._check(lib.silo_gpu_stream_read_probe(int(nbytes), 20, ctypes.byref(read_ms)))
        return round(read_ms.value, 4)

    with binding.GpuStore(n, [dict(name="main", alphabet="nuc", reference=reference)]) as store:
        store.generate_synthetic(0, model)
        store.finalize()
        row_words = store.row_words
        positions = len(reference)
        column_bytes = row_words * 64 * 4
        table = store.malloc(row_words * 64 * 16)
        table_scratch = store.malloc(binding.row_cell_count_scratch_bytes(positions))
        whole_ms = timed(lambda: binding._check(lib.silo_gpu_row_cell_counts(store.handle, 0, table, table_scratch, None)), args.build_reps)
        print(json.dumps({
            "sequences": n, "positions": positions, "row_cell_counts_ms": whole_ms, "plane_rows": store.scan_rows(0, 0, positions),
            "escape_keys": int(store.scan_escapes(0)), "runs": store.scan_runs(0), "sparse_keys": int(lib.silo_gpu_store_scan_sparse_keys(store.handle, 0)),
        }), flush=True)
        store.free(table)
        store.free(table_scratch)

        tiles = tiling(positions)
        chunks = colour(tiles)
        cases = {"1 position": [[(SPIKE[0] - 1, SPIKE[0])]], "24 positions": [[(SPIKE[0] - 1, SPIKE[0] + 23)]], "spike, 3 822 positions": [[(SPIKE[0] - 1, SPIKE[1])]],
                 "whole sequence": [[(0, positions)]], "98 tiling regions in %d colour classes" % len(chunks): [[tiles[g] for g in chunk] for chunk in chunks]}
        most = max(len(chunk) for chunk in chunks)
        columns = store.malloc(most * column_bytes)
        scratch = store.malloc(binding.region_value_scratch_bytes(positions))
        for name, calls in cases.items():
            arrays = [np.ascontiguousarray(ranges, dtype=np.uint32) for ranges in calls]

            def launches():
                for ranges in arrays:
                    binding._check(lib.silo_gpu_region_cell_values(store.handle, 0, binding._ptr(ranges), len(ranges), binding.CELL_COUNT_MISSING, columns, scratch, None))

            reps = args.build_reps if sum(end - first for ranges in calls for first, end in ranges) > 10_000 else args.reps
            ms = timed(launches, reps)
            touched = sum(store.scan_rows(0, first, end) for ranges in calls for first, end in ranges) * row_words * 8 + sum(len(ranges) for ranges in calls) * column_bytes
            print(json.dumps({
                "sequences": n, "entry": "region_cell_values", "case": name, "regions": sum(len(ranges) for ranges in calls), "calls": len(calls),
                "positions_walked": sum(end - first for ranges in calls for first, end in ranges), "ms": ms, "row_cell_counts_ms_same_run": whole_ms,
                "plane_and_column_bytes": touched, "stream_read_of_those_bytes_ms": stream_read_ms(touched),
            }), flush=True)

        # the readers, on the columns of the last call (the second colour class of the tiling)
        n_columns = len(chunks[-1])
        out = binding.device_malloc(row_words * 8)
        half = (tiles[chunks[-1][0]][1] - tiles[chunks[-1][0]][0]) // 2
        bitset_ms = timed(lambda: binding._check(lib.silo_gpu_bitset_from_values(columns, row_words, n, half, 0xFFFFFFFF, out, None)), args.reps)
        selected = int(np.unpackbits(binding.device_read(out, np.uint8, row_words * 8)).sum())
        bitset_bytes = column_bytes + row_words * 8
        print(json.dumps({
            "sequences": n, "kernel": "bitset_from_values", "at_least": half, "selected_rows": selected, "ms": bitset_ms,
            "bytes_read_and_written": bitset_bytes, "stream_read_of_those_bytes_ms": stream_read_ms(bitset_bytes),
        }), flush=True)
        binding.device_free(out)
        counts = binding.device_malloc(n_columns * 8, 0)
        filters = {"every row (NULL)": None, f"PangoLineage {bench.QUERY_LINEAGE}*": member[lineage]}
        for name, mask in filters.items():
            filter_dev = None if mask is None else binding._upload(words_of(mask, row_words))
            for used in (1, n_columns):
                bounds = np.ascontiguousarray([(half, 0xFFFFFFFF)] * used, dtype=np.uint32)
                ms = timed(lambda: binding._check(lib.silo_gpu_count_values(columns, used, row_words, n, filter_dev, binding._ptr(bounds), counts, None)), args.reps)
                rows = n if mask is None else int(mask.sum())
                read_bytes = used * 4 * rows + (0 if mask is None else used * row_words * 8)
                print(json.dumps({
                    "sequences": n, "kernel": "count_values", "filter": name, "filter_rows": rows, "columns": used, "ms": ms,
                    "bytes_read_at_least": read_bytes, "stream_read_of_those_bytes_ms": stream_read_ms(read_bytes),
                }), flush=True)
            if filter_dev is not None:
                binding.device_free(filter_dev)
        binding.device_free(counts)
        store.free(columns)
        store.free(scratch)


if __name__ == "__main__":
    main()
