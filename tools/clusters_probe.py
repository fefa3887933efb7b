#!/usr/bin/env python3
"""Clusters probe (K12): on bench.py's synthetic genome store (--sequences rows; a `key` and a `row` column are added so that rows
can be selected by number), for a contiguous selection of --rows rows (default 2 048):
  - silo_gpu_distance_within with no bound (early exit cannot fire), with maxDistance 2 and with maxDistance 10,
  - silo_gpu_distance_pairs on the same planes (K10's kernel: the yardstick),
  - silo_gpu_adjacency_components on the matrix of each bound, with its round count,
each between HIP events, medians of --reps runs after one that warms up; and one Clusters request against one
DistanceMatrix{maxDistance} request for the same rows, host clock around a request that ends in a fetch the host waits for,
response text included, not parsed, the two alternated.  Then the same Clusters request for --large-rows rows (default 8 192),
which DistanceMatrix refuses.  Prints one JSON line per measurement group; no ratio is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd"), os.path.join(ROOT, "tools")]

from distance_probe import build_engine  # noqa: E402

NO_BOUND = 0xFFFFFFFF


def timed(reps, call):
    """Median ms of `call` between two HIP events, after one run that warms up."""
    from silo_amd import binding

    times = []
    for _ in range(reps + 1):
        begin, end = binding.GpuEvent(), binding.GpuEvent()
        begin.record()
        call()
        end.record()
        times.append(begin.elapsed_ms(end))
    return round(float(np.median(times[1:])), 4)


def kernel_times(chars, reps):
    from silo_amd import binding

    lib = binding.load_library()
    n, positions = chars.shape
    planes_dev = binding.distance_pack_rows("nuc", chars)
    words = n * binding.adjacency_words(n)
    adjacency_dev = binding.device_malloc(words * 8)
    labels_dev = binding.device_malloc(n * 4)
    rounds_dev = binding.device_malloc(4)
    out = {}
    try:
        if n <= binding.MAX_DISTANCE_ROWS:
            table_dev = binding.device_malloc(n * n * 8)
            out["k_distance_pairs_ms"] = timed(reps, lambda: binding._check(lib.silo_gpu_distance_pairs(0, planes_dev, n, positions, table_dev, None)))
            binding.device_free(table_dev)
        for label, max_distance in (("no_bound", NO_BOUND), ("max_distance_2", 2), ("max_distance_10", 10)):
            out[f"distance_within_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_distance_within(0, planes_dev, n, positions, max_distance, 0, adjacency_dev, None)))
            out[f"components_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_adjacency_components(adjacency_dev, n, labels_dev, rounds_dev, None)))
            binding._check(lib.silo_gpu_stream_synchronize(None))
            out[f"components_{label}_rounds"] = int(binding.device_read(rounds_dev, np.uint32, 1)[0])
            out[f"links_{label}"] = int(np.bitwise_count(binding.device_read(adjacency_dev, np.uint64, words)).sum()) // 2
            out[f"clusters_{label}"] = len(np.unique(binding.device_read(labels_dev, np.uint32, n)))
    finally:
        for pointer in (planes_dev, adjacency_dev, labels_dev, rounds_dev):
            binding.device_free(pointer)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--rows", type=int, default=2048, help="selected sequences of the kernel timings and of the request pair")
    parser.add_argument("--large-rows", type=int, default=8192, help="selected sequences of the Clusters request alone")
    parser.add_argument("--max-distance", type=int, default=10, help="maxDistance of the requests")
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    t0 = time.perf_counter()
    engine = build_engine(args.sequences)
    build_s = time.perf_counter() - t0
    first = args.sequences // 3

    def request(action, n):
        return json.dumps({"action": action, "filterExpression": {"type": "IntBetween", "column": "row", "from": first, "to": first + n - 1}}).encode()

    def run(body):
        t = time.perf_counter()
        status, text = engine.execute_text(body)
        elapsed = (time.perf_counter() - t) * 1e3
        assert status == 200, text[:500]
        return elapsed, text

    n = args.rows
    clusters = request({"type": "Clusters", "maxDistance": args.max_distance}, n)
    matrix = request({"type": "DistanceMatrix", "maxDistance": args.max_distance}, n)
    _, clusters_body = run(clusters)
    _, matrix_body = run(matrix)
    _, fasta_body = run(request({"type": "FastaAligned", "sequenceName": "main"}, n))
    sequences = [row["main"] for row in json.loads(fasta_body.decode())["queryResult"]]
    chars = np.frombuffer("".join(sequences).encode(), dtype=np.uint8).reshape(n, -1)
    clusters_ms, matrix_ms = [], []
    for _ in range(args.reps):  # alternated, so that drift hits both
        clusters_ms.append(run(clusters)[0])
        matrix_ms.append(run(matrix)[0])
    print(json.dumps({
        "sequences": args.sequences, "selected": n, "positions": chars.shape[1], "build_s": round(build_s, 1), "max_distance": args.max_distance,
        "clusters_ms": [round(x, 3) for x in clusters_ms], "clusters_ms_median": round(float(np.median(clusters_ms)), 3),
        "clusters_response_bytes": len(clusters_body), "clusters_rows": clusters_body.count(b'"clusterSize":'),
        "distance_matrix_ms": [round(x, 3) for x in matrix_ms], "distance_matrix_ms_median": round(float(np.median(matrix_ms)), 3),
        "distance_matrix_response_bytes": len(matrix_body), "distance_matrix_rows": matrix_body.count(b'"distance":'),
        **kernel_times(chars, args.reps),
    }), flush=True)

    n = args.large_rows
    clusters = request({"type": "Clusters", "maxDistance": args.max_distance}, n)
    _, clusters_body = run(clusters)
    clusters_ms = [run(clusters)[0] for _ in range(args.reps)]
    print(json.dumps({
        "sequences": args.sequences, "selected": n, "max_distance": args.max_distance,
        "clusters_ms": [round(x, 3) for x in clusters_ms], "clusters_ms_median": round(float(np.median(clusters_ms)), 3),
        "clusters_response_bytes": len(clusters_body), "clusters_rows": clusters_body.count(b'"clusterSize":'),
    }), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
