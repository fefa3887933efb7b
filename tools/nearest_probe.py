#!/usr/bin/env python3
"""NearestNeighbours probe: a query by primary key under no filter and under the lineage filter of bench.py, on bench.py's
synthetic genome store (--sequences rows; a `key` column is added so that a row can be named).  Each request timing is a host
clock around a request that ends in a device -> host fetch the host waits for, response text included, not parsed; median of
--reps runs.  The passes are timed by themselves with HIP events: silo_gpu_query_distances as a whole (its launches follow one
another on one stream) and silo_gpu_nearest_rows, on a store of the same model built through the binding; and, beside them, the
one existing comparison point — an unfiltered Mutations scan of the same store (HIP events around silo_gpu_mutations_scan): the
same bytes, read once.  Prints one
JSON line per filter; no ratio is asserted."""
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
from distance_probe import build_engine  # noqa: E402


def pass_times(engine_query, positions, sequences, reps):
    """Medians of HIP event timings (ms) around the two entry points on a store of bench.py's model, and of a Mutations scan."""
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
        select_scratch = store.malloc(binding.NEAREST_ROWS_SCRATCH_BYTES)
        out = store.malloc(1024 * 12 + 4)
        counts = store.malloc(positions * 5 * 4)
        distances_ms, nearest_ms, scan_ms = [], [], []
        for _ in range(reps + 1):  # the first run warms up
            events = [binding.GpuEvent() for _ in range(4)]
            events[0].record()
            binding._check(lib.silo_gpu_query_distances(store.handle, 0, binding._ptr(query), table, scratch, None))
            events[1].record()
            binding._check(lib.silo_gpu_nearest_rows(table, None, sequences, binding.NO_ROW, binding.NO_ROW, 10, out,
                                                     ctypes_offset(out, 1024 * 12), select_scratch, None))
            events[2].record()
            store.memset(counts, 0, positions * 5 * 4)
            binding._check(lib.silo_gpu_mutations_scan(store.handle, 0, None, 0, positions, counts, None))
            events[3].record()
            store.synchronize()
            distances_ms.append(events[0].elapsed_ms(events[1]))
            nearest_ms.append(events[1].elapsed_ms(events[2]))
            scan_ms.append(events[2].elapsed_ms(events[3]))
    return tuple(float(np.median(values[1:])) for values in (distances_ms, nearest_ms, scan_ms))


def ctypes_offset(pointer, nbytes):
    return ctypes.c_void_p(pointer.value + nbytes)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--neighbours", type=int, default=10)
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
    distances_ms, nearest_ms, scan_ms = pass_times(query, len(query), args.sequences, args.reps)
    for name, expression in (("none", {"type": "True"}), ("lineage", {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True})):
        request = json.dumps({"action": {"type": "NearestNeighbours", "primaryKey": key, "neighbours": args.neighbours},
                              "filterExpression": expression}).encode()
        request_ms = []
        for _ in range(args.reps + 1):  # the first run warms up
            t = time.perf_counter()
            status, body = engine.execute_text(request)
            request_ms.append((time.perf_counter() - t) * 1e3)
            assert status == 200, body[:500]
        print(json.dumps({
            "sequences": args.sequences, "filter": name, "neighbours": args.neighbours, "returned": body.count(b'"distance":'),
            "positions": len(query), "build_s": round(build_s, 1),
            "nearest_neighbours_ms": [round(x, 3) for x in request_ms[1:]], "nearest_neighbours_ms_median": round(float(np.median(request_ms[1:])), 3),
            "query_distances_ms": round(distances_ms, 4), "nearest_rows_ms": round(nearest_ms, 4), "mutations_scan_ms": round(scan_ms, 4),
        }), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
