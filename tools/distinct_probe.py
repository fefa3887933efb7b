#!/usr/bin/env python3
"""DistinctSequences probe (K20): bench.py's synthetic genome store (--sequences rows, one partition) built through the binding, the
filter of all rows and the row set of bench.py's lineage filter (QUERY_LINEAGE with sublineages).  HIP events on the null stream,
median of --reps runs behind one warm-up each (--hash-reps for the one-time table):
  - silo_gpu_row_hashes as a whole: its table upload, the plane pass and the key, run and sparse passes behind it on one stream
    (the passes by themselves are read off a kernel trace of this program: rocprofv3 --kernel-trace --stats);
  - silo_gpu_distinct_begin + _insert + _select under each filter, on the hashes that call left;
  - silo_gpu_stream_read_probe over the bytes the plane pass reads (the store's planes) and over the bytes a selection reads at
    the least (the bitset twice, 16 bytes of hash per selected row twice, the owner table once).
--engine instead times `Aggregated` requests through the engine on the same store: under the child alone, the FIRST request under
DistinctSequences of it on a fresh store (which computes the kept hashes), and the later ones.
Prints one JSON line per case; no ratio is asserted."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd")]

import bench  # noqa: E402


def words_of(mask, row_words):
    padded = np.zeros(row_words * 64, dtype=bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


def synthetic_model(n):
    from silo_amd import alphabet, synth

    genomes = bench.load_reference_genomes(False)
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in genomes["nucleotideSequences"][0]["sequence"]], dtype=np.uint8)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n, tree, synth.DEFAULT_SEED)
    model = synth.make_model(n, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    return genomes, reference, tree, lineage, model


def through_the_engine(args):
    """--engine: the host clock around `Aggregated` requests.  One JSON line per child; a fresh engine per child, so that the first
    request under DistinctSequences finds a store without hashes."""
    from silo_amd.engine import Engine

    n = args.sequences
    genomes, _, tree, lineage, model = synthetic_model(n)
    children = {"True": {"type": "True"},
                f"PangoLineage {bench.QUERY_LINEAGE}*": {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}}
    for name, child in children.items():
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

        child_times = [request_ms(child) for _ in range(args.reps + 1)]
        distinct = {"type": "DistinctSequences", "child": child}
        first_ms, distinct_rows = request_ms(distinct)
        later = [request_ms(distinct)[0] for _ in range(args.reps)]
        print(json.dumps({
            "sequences": n, "child": name, "child_rows": child_times[0][1], "aggregated_under_child_ms": round(float(np.median([t for t, _ in child_times[1:]])), 4),
            "first_aggregated_under_distinct_ms": round(first_ms, 4), "aggregated_under_distinct_ms": round(float(np.median(later)), 4),
            "distinct_rows": distinct_rows,
        }), flush=True)
        engine.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--hash-reps", type=int, default=20)
    parser.add_argument("--engine", action="store_true", help="time requests through the engine instead of the C entries")
    args = parser.parse_args()
    if args.engine:
        return through_the_engine(args)

    from silo_amd import binding

    lib = binding.load_library()
    n = args.sequences
    _, reference, tree, lineage, model = synthetic_model(n)
    member = tree.subtree(tree.names.index(bench.QUERY_LINEAGE)).astype(bool)
    filters = {"True": np.ones(n, dtype=bool), f"PangoLineage {bench.QUERY_LINEAGE}*": member[lineage]}

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
        hashes = store.malloc(row_words * 64 * 16)
        scratch = store.malloc(binding.row_hash_scratch_bytes(positions))
        hashes_ms = timed(lambda: binding._check(lib.silo_gpu_row_hashes(store.handle, 0, hashes, scratch, None)), args.hash_reps)
        plane_bytes = store.scan_rows(0, 0, positions) * row_words * 8
        print(json.dumps({
            "sequences": n, "positions": positions, "row_hashes_ms": hashes_ms, "plane_rows": store.scan_rows(0, 0, positions), "plane_bytes": plane_bytes,
            "escape_keys": int(store.scan_escapes(0)), "runs": store.scan_runs(0), "sparse_keys": int(lib.silo_gpu_store_scan_sparse_keys(store.handle, 0)),
            "stream_read_of_the_planes_ms": stream_read_ms(plane_bytes), "table_bytes": row_words * 64 * 16,
        }), flush=True)

        slots = binding.distinct_slots(n)
        table = binding.device_malloc(binding.distinct_table_bytes(slots))
        out = binding.device_malloc(row_words * 8)
        record = np.zeros(1, dtype=binding.DISTINCT_PART_DTYPE)
        record[0] = (hashes.value, 0, n, row_words, 0)
        parts = binding._upload(record)
        for name, mask in filters.items():
            filter_dev = binding._upload(words_of(mask, row_words))

            def selection():
                binding._check(lib.silo_gpu_distinct_begin(table, slots, None))
                binding._check(lib.silo_gpu_distinct_insert(table, slots, parts, 1, 0, filter_dev, None))
                binding._check(lib.silo_gpu_distinct_select(table, slots, parts, 1, 0, filter_dev, out, None))

            selection_ms = timed(selection, args.reps)
            begin_ms = timed(lambda: binding._check(lib.silo_gpu_distinct_begin(table, slots, None)), args.reps)
            selected = int(np.unpackbits(binding.device_read(out, np.uint8, row_words * 8)).sum())
            overflow = int(binding.device_read(table, np.uint32, slots + 1)[-1])
            least_bytes = 2 * row_words * 8 + 2 * 16 * int(mask.sum()) + binding.distinct_table_bytes(slots)
            print(json.dumps({
                "sequences": n, "filter": name, "filter_rows": int(mask.sum()), "slots": slots, "distinct_rows": selected, "overflow": overflow,
                "begin_insert_select_ms": selection_ms, "begin_ms": begin_ms, "bytes_read_at_least": least_bytes,
                "stream_read_of_those_bytes_ms": stream_read_ms(least_bytes),
            }), flush=True)
            binding.device_free(filter_dev)
        for ptr in (table, out, parts):
            binding.device_free(ptr)
        store.free(hashes)
        store.free(scratch)


if __name__ == "__main__":
    main()
