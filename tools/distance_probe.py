#!/usr/bin/env python3
"""DistanceMatrix probe: the action for selections of 256, 1 024 and 2 048 rows against a FastaAligned request for the same rows
— what a client has to fetch today before it can compare anything, and the only baseline the engine offered before — on
bench.py's synthetic genome store (--sequences rows; a `key` and a `row` column are added so that rows can be selected by
number).  Each request timing is a host clock around a request that ends in a device -> host fetch the host waits for, response
text included, not parsed; medians of --reps runs, the two requests alternated.  The kernels are timed by themselves with HIP
events around silo_gpu_distance_pack and silo_gpu_distance_pairs on the characters of the FastaAligned response.  Prints one
JSON line per selection; no ratio is asserted."""
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


def build_engine(n_sequences):
    """bench.build_engine's store (same lineage tree, model and seed) with a primary key and a row number column."""
    from silo_amd import alphabet, synth
    from silo_amd.engine import Engine

    genomes = bench.load_reference_genomes(False)
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in genomes["nucleotideSequences"][0]["sequence"]], dtype=np.uint8)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n_sequences, tree, synth.DEFAULT_SEED)
    model = synth.make_model(n_sequences, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    engine = Engine(genomes)
    engine.set_schema("key", None)
    partition = engine.add_partition(n_sequences)
    engine.generate_synthetic(partition, "main", False, model, engine.position_window("main", False))
    engine.set_lineage_column_ids(partition, "pango_lineage", tree.names, lineage)
    engine.append_metadata(partition, "key", "string", [f"S{i}" for i in range(n_sequences)])
    engine.append_metadata(partition, "row", "int", [str(i) for i in range(n_sequences)])
    engine.finalize()
    return engine


def kernel_times(chars, reps):
    """(pack ms, pairs ms): medians of HIP event timings around the two entry points alone."""
    from silo_amd import binding

    lib = binding.load_library()
    n, positions = chars.shape
    chars_dev = binding.device_malloc(chars.size)
    planes_dev = binding.device_malloc(n * binding.distance_planes("nuc") * binding.distance_words(positions) * 8)
    table_dev = binding.device_malloc(n * n * 8)
    binding._check(lib.silo_gpu_memcpy_h2d(chars_dev, chars.ctypes.data_as(ctypes.c_void_p), chars.size, None))
    pack_ms, pairs_ms = [], []
    for _ in range(reps + 1):  # the first run warms up
        events = [binding.GpuEvent() for _ in range(3)]
        events[0].record()
        binding._check(lib.silo_gpu_distance_pack(0, chars_dev, n, positions, planes_dev, None))
        events[1].record()
        binding._check(lib.silo_gpu_distance_pairs(0, planes_dev, n, positions, table_dev, None))
        events[2].record()
        pack_ms.append(events[0].elapsed_ms(events[1]))
        pairs_ms.append(events[1].elapsed_ms(events[2]))
    for pointer in (chars_dev, planes_dev, table_dev):
        binding.device_free(pointer)
    return float(np.median(pack_ms[1:])), float(np.median(pairs_ms[1:]))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--rows", type=int, nargs="+", default=[256, 1024, 2048], help="selected sequences; one measurement each")
    parser.add_argument("--max-distance", type=int, default=None, help="maxDistance of the request (default: every pair is returned)")
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    t0 = time.perf_counter()
    engine = build_engine(args.sequences)
    build_s = time.perf_counter() - t0
    for n in args.rows:
        first = args.sequences // 3
        selection = {"type": "IntBetween", "column": "row", "from": first, "to": first + n - 1}
        action = {"type": "DistanceMatrix"}
        if args.max_distance is not None:
            action["maxDistance"] = args.max_distance
        distance = json.dumps({"action": action, "filterExpression": selection}).encode()
        fasta = json.dumps({"action": {"type": "FastaAligned", "sequenceName": "main"}, "filterExpression": selection}).encode()

        def run(request):
            t = time.perf_counter()
            status, body = engine.execute_text(request)
            elapsed = (time.perf_counter() - t) * 1e3
            assert status == 200, body[:500]
            return elapsed, body

        _, distance_body = run(distance)
        _, fasta_body = run(fasta)
        sequences = [row["main"] for row in json.loads(fasta_body.decode())["queryResult"]]
        chars = np.frombuffer("".join(sequences).encode(), dtype=np.uint8).reshape(n, -1)
        distance_ms, fasta_ms = [], []
        for _ in range(args.reps):  # alternated, so that drift hits both
            distance_ms.append(run(distance)[0])
            fasta_ms.append(run(fasta)[0])
        pack_ms, pairs_ms = kernel_times(chars, args.reps)
        print(json.dumps({
            "sequences": args.sequences, "selected": n, "positions": chars.shape[1], "build_s": round(build_s, 1),
            "pairs_returned": distance_body.count(b'"distance":'), "max_distance": args.max_distance,
            "distance_matrix_ms": [round(x, 3) for x in distance_ms], "distance_matrix_ms_median": round(float(np.median(distance_ms)), 3),
            "distance_matrix_response_bytes": len(distance_body),
            "fasta_aligned_ms": [round(x, 3) for x in fasta_ms], "fasta_aligned_ms_median": round(float(np.median(fasta_ms)), 3),
            "fasta_aligned_response_bytes": len(fasta_body),
            "k_distance_pack_ms": round(pack_ms, 4), "k_distance_pairs_ms": round(pairs_ms, 4),
        }), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
