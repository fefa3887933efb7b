#!/usr/bin/env python3
"""CellCount probe (K22): bench.py's synthetic genome store (--sequences rows, one partition) built through the binding.  HIP events
on the null stream, median of --reps runs behind one warm-up each (--build-reps for the one-time tables):
  - silo_gpu_row_cell_counts as a whole: its table upload, the plane pass and the key, run and sparse passes behind it on one
    stream; beside it silo_gpu_row_hashes (K20) on the same store, whose plane pass multiplies where this one compares;
  - silo_gpu_bitset_from_cell_counts alone and silo_gpu_cell_count_histogram alone (all rows, and bench.py's lineage filter), on the
    table that call left, against silo_gpu_stream_read_probe over the bytes each must read: 16 bytes per row, plus the filter.
--engine instead times `Aggregated` requests through the engine on the same store: the FIRST request under CellCount{missing, atMost}
on a fresh store (which computes the kept table), the later ones, and the stand-in it replaces: WithinDistance with the reference as
the literal query, the largest maxDistance it accepts and minComparedPositions.
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


def through_the_engine(args):
    """--engine: the host clock around `Aggregated` requests, one JSON line."""
    from silo_amd.engine import Engine

    n = args.sequences
    genomes, _, tree, lineage, model = synthetic_model(n)
    reference_text = genomes["nucleotideSequences"][0]["sequence"]
    positions = len(reference_text)
    engine = Engine(genomes)
    engine.set_schema("key", None)
    partition = engine.add_partition(n)
    engine.generate_synthetic(partition, "main", False, model, engine.position_window("main", False))
    engine.set_lineage_column_ids(partition, "pango_lineage", tree.names, lineage)
    engine.append_metadata(partition, "key", "string", [f"S{i}" for i in range(n)])
    engine.finalize()

    def request_ms(expression):
        request = json.dumps({"action": {"type": "Aggregated"}, "filterExpression": expression}).encode()
        t = time.perf_counter()
        status, body = engine.execute_text(request)
        elapsed = (time.perf_counter() - t) * 1e3
        assert status == 200, body[:500]
        return elapsed, json.loads(body.decode())["queryResult"][0]["count"]

    at_most = args.at_most
    bounded = {"type": "CellCount", "cells": "missing", "atMost": at_most}
    first_ms, rows = request_ms(bounded)
    later = [request_ms(bounded)[0] for _ in range(args.reps)]
    stand_in = {"type": "WithinDistance", "sequence": reference_text, "maxDistance": 2**31 - 1, "minComparedPositions": positions - at_most}
    stand_in_times = [request_ms(stand_in) for _ in range(args.reps + 1)]
    histogram_request = json.dumps({"action": {"type": "CellCountDistribution", "cells": "missing", "binWidth": 100}, "filterExpression": {"type": "True"}}).encode()
    histogram_times = []
    for _ in range(args.reps + 1):
        t = time.perf_counter()
        status, body = engine.execute_text(histogram_request)
        histogram_times.append((time.perf_counter() - t) * 1e3)
        assert status == 200, body[:500]
    print(json.dumps({
        "sequences": n, "positions": positions, "at_most_missing": at_most, "rows": rows,
        "first_aggregated_under_cell_count_ms": round(first_ms, 4), "aggregated_under_cell_count_ms": round(float(np.median(later)), 4),
        "aggregated_under_within_distance_ms": round(float(np.median([t for t, _ in stand_in_times[1:]])), 4), "within_distance_rows": stand_in_times[0][1],
        "cell_count_distribution_ms": round(float(np.median(histogram_times[1:])), 4),
    }), flush=True)
    engine.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--build-reps", type=int, default=5)
    parser.add_argument("--at-most", type=int, default=3000, help="the bound on the missing cells of the requests and of the bitset")
    parser.add_argument("--engine", action="store_true", help="time requests through the engine instead of the C entries")
    args = parser.parse_args()
    if args.engine:
        return through_the_engine(args)

    from silo_amd import binding

    lib = binding.load_library()
    n = args.sequences
    _, reference, tree, lineage, model = synthetic_model(n)
    member = tree.subtree(tree.names.index(bench.QUERY_LINEAGE)).astype(bool)
    filters = {"every row (NULL)": None, "True": np.ones(n, dtype=bool), f"PangoLineage {bench.QUERY_LINEAGE}*": member[lineage]}

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
        table = store.malloc(row_words * 64 * 16)
        scratch = store.malloc(binding.row_cell_count_scratch_bytes(positions))
        hashes = store.malloc(row_words * 64 * 16)
        hash_scratch = store.malloc(binding.row_hash_scratch_bytes(positions))
        hashes_ms = timed(lambda: binding._check(lib.silo_gpu_row_hashes(store.handle, 0, hashes, hash_scratch, None)), args.build_reps)
        counts_ms = timed(lambda: binding._check(lib.silo_gpu_row_cell_counts(store.handle, 0, table, scratch, None)), args.build_reps)
        plane_bytes = store.scan_rows(0, 0, positions) * row_words * 8
        print(json.dumps({
            "sequences": n, "positions": positions, "row_cell_counts_ms": counts_ms, "row_hashes_ms": hashes_ms,
            "plane_rows": store.scan_rows(0, 0, positions), "plane_bytes": plane_bytes, "escape_keys": int(store.scan_escapes(0)), "runs": store.scan_runs(0),
            "sparse_keys": int(lib.silo_gpu_store_scan_sparse_keys(store.handle, 0)), "stream_read_of_the_planes_ms": stream_read_ms(plane_bytes),
            "table_bytes": row_words * 64 * 16,
        }), flush=True)
        store.free(hashes)
        store.free(hash_scratch)

        out = binding.device_malloc(row_words * 8)
        bitset_ms = timed(lambda: binding._check(lib.silo_gpu_bitset_from_cell_counts(table, row_words, n, binding.CELL_COUNT_MISSING, 0, args.at_most, out, None)),
                          args.reps)
        selected = int(np.unpackbits(binding.device_read(out, np.uint8, row_words * 8)).sum())
        bitset_bytes = row_words * 64 * 16 + row_words * 8
        print(json.dumps({
            "sequences": n, "kernel": "bitset_from_cell_counts", "at_most_missing": args.at_most, "selected_rows": selected, "ms": bitset_ms,
            "bytes_read_and_written": bitset_bytes, "stream_read_of_those_bytes_ms": stream_read_ms(bitset_bytes),
        }), flush=True)
        binding.device_free(out)

        n_bins = 1024
        bins = binding.device_malloc(n_bins * 8, 0)
        for name, mask in filters.items():
            filter_dev = None if mask is None else binding._upload(words_of(mask, row_words))
            for bin_width in (1, 100):
                histogram_ms = timed(lambda: binding._check(lib.silo_gpu_cell_count_histogram(
                    table, row_words, n, filter_dev, binding.CELL_COUNT_MISSING, bin_width, n_bins, bins, None)), args.reps)
                rows = n if mask is None else int(mask.sum())
                read_bytes = 16 * rows + (0 if mask is None else row_words * 8)
                print(json.dumps({
                    "sequences": n, "kernel": "cell_count_histogram", "filter": name, "filter_rows": rows, "bin_width": bin_width, "n_bins": n_bins, "ms": histogram_ms,
                    "bytes_read_at_least": read_bytes, "stream_read_of_those_bytes_ms": stream_read_ms(read_bytes),
                }), flush=True)
            if filter_dev is not None:
                binding.device_free(filter_dev)
        binding.device_free(bins)
        store.free(table)
        store.free(scratch)


if __name__ == "__main__":
    main()
