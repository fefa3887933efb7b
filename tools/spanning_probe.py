#!/usr/bin/env python3
"""MinimumSpanningTree probe (K13): on bench.py's synthetic genome store (--sequences rows; a `key` and a `row` column are added so
that rows can be selected by number), for contiguous selections of --rows rows (default 2 048 and 8 192), with no bound and with
--max-distance (default 10):
  - silo_gpu_distance_weights, silo_gpu_spanning_forest on its matrix and silo_gpu_distance_listed_pairs on the forest's keys,
each between HIP events, medians of --reps runs after one that warms up; and one MinimumSpanningTree request without a bound, one
with maxDistance, one Clusters{maxDistance} request and — up to the 2 048 rows it takes — one DistanceMatrix request (what a client
that builds the tree itself fetches today) for the same rows: host clock around a request that ends in a fetch the host waits for,
response text included, not parsed, the requests alternated.  Prints one JSON line per selection; no ratio is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd"), os.path.join(ROOT, "tools")]

from clusters_probe import timed  # noqa: E402
from distance_probe import build_engine  # noqa: E402

NO_BOUND = 0xFFFFFFFF


def kernel_times(chars, reps, max_distance):
    from silo_amd import binding

    lib = binding.load_library()
    n, positions = chars.shape
    planes_dev = binding.distance_pack_rows("nuc", chars)
    weights_dev = binding.device_malloc(n * n * 4)
    edges_dev = binding.device_malloc(max(n - 1, 1) * 8)
    count_dev = binding.device_malloc(4)
    pairs_dev = binding.device_malloc(max(n - 1, 1) * 8)
    out = {}
    try:
        for label, bound in (("no_bound", NO_BOUND), (f"max_distance_{max_distance}", max_distance)):
            out[f"distance_weights_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_distance_weights(0, planes_dev, n, positions, bound, 0, weights_dev, None)))
            out[f"spanning_forest_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_spanning_forest(weights_dev, n, edges_dev, count_dev, None)))
            out[f"listed_pairs_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_distance_listed_pairs(0, planes_dev, n, positions, edges_dev, count_dev, n - 1, pairs_dev, None)))
            binding._check(lib.silo_gpu_stream_synchronize(None))
            out[f"edges_{label}"] = int(binding.device_read(count_dev, np.uint32, 1)[0])
    finally:
        for pointer in (planes_dev, weights_dev, edges_dev, count_dev, pairs_dev):
            binding.device_free(pointer)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--rows", type=int, nargs="+", default=[2048, 8192], help="selected sequences, one line of output each")
    parser.add_argument("--max-distance", type=int, default=10, help="maxDistance of the bounded requests")
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    from silo_amd import binding

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

    for n in args.rows:
        requests = {
            "tree": request({"type": "MinimumSpanningTree"}, n),
            "tree_bounded": request({"type": "MinimumSpanningTree", "maxDistance": args.max_distance}, n),
            "clusters": request({"type": "Clusters", "maxDistance": args.max_distance}, n),
        }
        if n <= binding.MAX_DISTANCE_ROWS:
            requests["distance_matrix"] = request({"type": "DistanceMatrix"}, n)
        bodies = {label: run(body)[1] for label, body in requests.items()}  # warms up
        times = {label: [] for label in requests}
        for _ in range(args.reps):  # alternated, so that drift hits all
            for label, body in requests.items():
                times[label].append(run(body)[0])
        line = {"sequences": args.sequences, "selected": n, "build_s": round(build_s, 1), "max_distance": args.max_distance}
        for label in requests:
            line[f"{label}_ms"] = [round(x, 3) for x in times[label]]
            line[f"{label}_ms_median"] = round(float(np.median(times[label])), 3)
            line[f"{label}_response_bytes"] = len(bodies[label])
            line[f"{label}_rows"] = bodies[label].count(b'"clusterSize":' if label == "clusters" else b'"distance":')
        # the characters of the same rows for the kernel timings, in pieces FastaAligned takes
        sequences = []
        for begin in range(0, n, 2048):
            body = json.dumps({"action": {"type": "FastaAligned", "sequenceName": "main"},
                               "filterExpression": {"type": "IntBetween", "column": "row", "from": first + begin, "to": first + min(begin + 2048, n) - 1}}).encode()
            sequences += [row["main"] for row in json.loads(run(body)[1].decode())["queryResult"]]
        chars = np.frombuffer("".join(sequences).encode(), dtype=np.uint8).reshape(n, -1)
        line["positions"] = chars.shape[1]
        line.update(kernel_times(chars, args.reps, args.max_distance))
        print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
