#!/usr/bin/env python3
"""WithinDistance probe, on bench.py's synthetic genome store (--sequences rows; a `key` column is added so that a row can be
named).  Three clocks, median of --reps runs each:
  - the host clock around one `Aggregated` request under `WithinDistance` by primary key (response text included, not parsed);
  - the same clock around the round trip that the expression replaces: a `NearestNeighbours` request (--neighbours rows, the same
    bound), its response parsed, and an `Aggregated` request under the `Or` of `StringEquals` of the returned keys and the key;
  - HIP events around silo_gpu_bitset_from_distances alone, on a table that silo_gpu_query_distances wrote for a store of the
    same model built through the binding.
The two requests are compared only where NearestNeighbours returned every row within the bound (fewer than --neighbours): the
line says so.  Prints one JSON line per bound; no ratio is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd"), os.path.join(ROOT, "tools")]

import bench  # noqa: E402
from distance_probe import build_engine  # noqa: E402


def kernel_ms(engine_query, positions, sequences, bounds, reps):
    """Per bound: (median of HIP event timings (ms) around silo_gpu_bitset_from_distances, rows selected) on a store of bench.py's model."""
    from silo_amd import alphabet, binding, synth

    genomes = bench.load_reference_genomes(False)
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in genomes["nucleotideSequences"][0]["sequence"]], dtype=np.uint8)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(sequences, tree, synth.DEFAULT_SEED)
    model = synth.make_model(sequences, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    lib = binding.load_library()
    with binding.GpuStore(sequences, [dict(name="main", alphabet="nuc", reference=reference)]) as store:
        store.generate_synthetic(0, model)
        store.finalize()
        query = np.frombuffer(engine_query.encode(), dtype=np.uint8)
        table = store.malloc(store.row_words * 64 * 8)
        scratch = store.malloc(binding.query_distance_scratch_bytes(positions))
        bitset = store.malloc(store.row_words * 8)
        binding._check(lib.silo_gpu_query_distances(store.handle, 0, binding._ptr(query), table, scratch, None))
        results = {}
        for max_distance in bounds:
            times = []
            for _ in range(reps + 1):  # the first run warms up
                events = [binding.GpuEvent() for _ in range(2)]
                events[0].record()
                binding._check(lib.silo_gpu_bitset_from_distances(table, sequences, store.row_words, max_distance, 0, bitset, None))
                events[1].record()
                store.synchronize()
                times.append(events[0].elapsed_ms(events[1]))
            selected = int(np.unpackbits(binding.device_read(bitset, np.uint8, store.row_words * 8)).sum())
            results[max_distance] = (float(np.median(times[1:])), selected)
    return results


def timed(engine, request):
    t = time.perf_counter()
    status, body = engine.execute_text(request)
    elapsed = (time.perf_counter() - t) * 1e3
    assert status == 200, body[:500]
    return elapsed, body


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--neighbours", type=int, default=1024)
    parser.add_argument("--bounds", type=int, nargs="+", default=[2, 10])
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    t0 = time.perf_counter()
    engine = build_engine(args.sequences)
    build_s = time.perf_counter() - t0
    key = f"S{args.sequences // 3}"
    status, body = engine.execute_text(json.dumps({"action": {"type": "FastaAligned", "sequenceName": "main"},
                                                   "filterExpression": {"type": "StringEquals", "column": "key", "value": key}}).encode())
    assert status == 200, body[:500]
    query = json.loads(body.decode())["queryResult"][0]["main"]
    kernel = kernel_ms(query, len(query), args.sequences, args.bounds, args.reps)
    for bound in args.bounds:
        within = json.dumps({"action": {"type": "Aggregated"},
                             "filterExpression": {"type": "WithinDistance", "primaryKey": key, "maxDistance": bound}}).encode()
        nearest = json.dumps({"action": {"type": "NearestNeighbours", "primaryKey": key, "neighbours": args.neighbours, "maxDistance": bound},
                              "filterExpression": {"type": "True"}}).encode()
        within_ms, round_trip_ms = [], []
        for _ in range(args.reps + 1):  # the first run warms up
            elapsed, body = timed(engine, within)
            within_ms.append(elapsed)
            within_count = json.loads(body.decode())["queryResult"][0]["count"]
            t = time.perf_counter()
            _, body = timed(engine, nearest)
            keys = [entry["primaryKey"] for entry in json.loads(body.decode())["queryResult"]] + [key]
            pasted = json.dumps({"action": {"type": "Aggregated"}, "filterExpression": {"type": "Or", "children": [
                {"type": "StringEquals", "column": "key", "value": value} for value in keys]}}).encode()
            _, body = timed(engine, pasted)
            round_trip_ms.append((time.perf_counter() - t) * 1e3)
            pasted_count = json.loads(body.decode())["queryResult"][0]["count"]
        event_ms, selected = kernel[bound]
        print(json.dumps({
            "sequences": args.sequences, "positions": len(query), "max_distance": bound, "build_s": round(build_s, 1),
            "within_distance_count": within_count, "round_trip_count": pasted_count, "round_trip_complete": pasted_count == within_count,
            "aggregated_under_within_distance_ms": [round(x, 3) for x in within_ms[1:]],
            "aggregated_under_within_distance_ms_median": round(float(np.median(within_ms[1:])), 3),
            "nearest_neighbours_then_or_of_keys_ms": [round(x, 3) for x in round_trip_ms[1:]],
            "nearest_neighbours_then_or_of_keys_ms_median": round(float(np.median(round_trip_ms[1:])), 3),
            "bitset_from_distances_ms": round(event_ms, 4), "bitset_from_distances_selected": selected,
        }), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
