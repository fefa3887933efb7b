#!/usr/bin/env python3
"""NearestAmong probe (K14): on bench.py's synthetic genome store (--sequences rows; a `key` and a `row` column are added so that
rows can be selected by number), for --shapes subjects x candidates (default 64 x 8 192, 2 048 x 8 192 and 1 024 x 1 024; two
contiguous stretches of rows that do not overlap), with no bound and with --max-distance (default 10):
  - silo_gpu_distance_cross and silo_gpu_nearest_columns on its cells,
each between HIP events, medians of --reps runs after one that warms up; one NearestAmong request without a bound and one with
maxDistance; and what a client does today for the same rows: one NearestNeighbours request per subject under the candidates' filter
(all of them where there are at most --nn-all subjects, a sample of that many spread over the subjects otherwise: then only the time
per request is measured, not the total) and — where the union is at most the 2 048 rows it takes — one DistanceMatrix request of
the union.  Host clock around a request that ends in a fetch the host waits for, response text included, not parsed, the requests
alternated.  Prints one JSON line per shape; no ratio is asserted."""
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


def kernel_times(subject_chars, candidate_chars, neighbours, reps, max_distance):
    from silo_amd import binding

    lib = binding.load_library()
    m, positions = subject_chars.shape
    n = len(candidate_chars)
    rows_dev = binding.distance_pack_rows("nuc", subject_chars)
    columns_dev = binding.distance_pack_rows("nuc", candidate_chars)
    cells_dev = binding.device_malloc(m * n * 8)
    lists_dev = binding.device_malloc(m * neighbours * 12)
    counts_dev = binding.device_malloc(m * 4)
    out = {}
    try:
        for label, bound in (("no_bound", NO_BOUND), (f"max_distance_{max_distance}", max_distance)):
            out[f"distance_cross_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_distance_cross(0, rows_dev, m, columns_dev, n, positions, None, bound, 0, cells_dev, None)))
            out[f"nearest_columns_{label}_ms"] = timed(
                reps, lambda: binding._check(lib.silo_gpu_nearest_columns(cells_dev, m, n, neighbours, lists_dev, counts_dev, None)))
            binding._check(lib.silo_gpu_stream_synchronize(None))
            out[f"listed_{label}"] = int(binding.device_read(counts_dev, np.uint32, m).sum())
    finally:
        for pointer in (rows_dev, columns_dev, cells_dev, lists_dev, counts_dev):
            binding.device_free(pointer)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--shapes", nargs="+", default=["64x8192", "2048x8192", "1024x1024"], help="subjects x candidates, one line of output each")
    parser.add_argument("--neighbours", type=int, default=10)
    parser.add_argument("--max-distance", type=int, default=10, help="maxDistance of the bounded requests")
    parser.add_argument("--nn-all", type=int, default=64, help="subjects up to which every NearestNeighbours request is made; above: a sample of that many")
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    from silo_amd import binding

    t0 = time.perf_counter()
    engine = build_engine(args.sequences)
    build_s = time.perf_counter() - t0
    print(f"store of {args.sequences} rows built in {build_s:.1f} s", file=sys.stderr, flush=True)

    def stretch(first, count):
        return {"type": "IntBetween", "column": "row", "from": first, "to": first + count - 1}

    def run(body):
        t = time.perf_counter()
        status, text = engine.execute_text(body)
        elapsed = (time.perf_counter() - t) * 1e3
        assert status == 200, text[:500]
        return elapsed, text

    def characters(first, count):
        """The characters of the rows for the kernel timings, in pieces FastaAligned takes."""
        sequences = []
        for begin in range(0, count, 2048):
            body = json.dumps({"action": {"type": "FastaAligned", "sequenceName": "main"}, "filterExpression": stretch(first + begin, min(2048, count - begin))}).encode()
            sequences += [row["main"] for row in json.loads(run(body)[1].decode())["queryResult"]]
        return np.frombuffer("".join(sequences).encode(), dtype=np.uint8).reshape(count, -1)

    for shape in args.shapes:
        m, n = (int(side) for side in shape.split("x"))
        first_subject, first_candidate = args.sequences // 3, 2 * args.sequences // 3
        assert first_subject + m <= first_candidate and first_candidate + n <= args.sequences
        subjects, candidates = stretch(first_subject, m), stretch(first_candidate, n)
        action = {"type": "NearestAmong", "among": candidates, "neighbours": args.neighbours}
        requests = {
            "nearest_among": json.dumps({"action": action, "filterExpression": subjects}).encode(),
            "nearest_among_bounded": json.dumps({"action": dict(action, maxDistance=args.max_distance), "filterExpression": subjects}).encode(),
        }
        if m + n <= binding.MAX_DISTANCE_ROWS:
            requests["distance_matrix_of_the_union"] = json.dumps({"action": {"type": "DistanceMatrix"}, "filterExpression": {"type": "Or", "children": [subjects, candidates]}}).encode()
        bodies = {label: run(body)[1] for label, body in requests.items()}  # warms up
        times = {label: [] for label in requests}
        for _ in range(args.reps):  # alternated, so that drift hits all
            for label, body in requests.items():
                times[label].append(run(body)[0])
        line = {"sequences": args.sequences, "subjects": m, "candidates": n, "neighbours": args.neighbours, "build_s": round(build_s, 1), "max_distance": args.max_distance}
        for label in requests:
            line[f"{label}_ms"] = [round(x, 3) for x in times[label]]
            line[f"{label}_ms_median"] = round(float(np.median(times[label])), 3)
            line[f"{label}_response_bytes"] = len(bodies[label])
            line[f"{label}_rows"] = bodies[label].count(b'"distance":')
        # what a client does today: one NearestNeighbours request per subject, under the candidates' filter
        asked = list(range(m)) if m <= args.nn_all else [int(s) for s in np.linspace(0, m - 1, args.nn_all)]
        for label, fields in (("nearest_neighbours", {}), ("nearest_neighbours_bounded", {"maxDistance": args.max_distance})):
            neighbour_requests = [
                json.dumps({"action": dict(fields, type="NearestNeighbours", primaryKey=f"S{first_subject + s}", neighbours=args.neighbours), "filterExpression": candidates}).encode()
                for s in asked
            ]
            totals, each, size = [], [], 0
            for rep in range(args.reps + 1):  # the first round warms up
                t = time.perf_counter()
                answers = [run(body) for body in neighbour_requests]
                if rep:
                    totals.append((time.perf_counter() - t) * 1e3)
                    each += [elapsed for elapsed, _ in answers]
                size = sum(len(text) for _, text in answers)
            line[f"{label}_requests_made"] = len(asked)
            line[f"{label}_ms_per_request_median"] = round(float(np.median(each)), 3)
            line[f"{label}_response_bytes_of_those"] = size
            # the total of all m requests is a measurement only where all m were made
            line[f"{label}_all_subjects_ms_median"] = round(float(np.median(totals)), 3) if len(asked) == m else "not measured"
        subject_chars, candidate_chars = characters(first_subject, m), characters(first_candidate, n)
        line["positions"] = subject_chars.shape[1]
        line.update(kernel_times(subject_chars, candidate_chars, args.neighbours, args.reps, args.max_distance))
        print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
