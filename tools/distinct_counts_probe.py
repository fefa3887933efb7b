#!/usr/bin/env python3
"""DistinctSequenceCounts probe (K21): bench.py's synthetic genome store (--sequences rows, one partition) built through the binding,
as tools/distinct_probe.py builds it.  HIP events on the null stream, median of --reps runs behind one warm-up each.  Under the
filter of all rows, under the row set of bench.py's lineage filter (QUERY_LINEAGE with sublineages), under the rows of the store's
LARGEST class (found with the chain itself), and — the worst case, which the synthetic store does not hold — on a table of hashes
that are all equal, so that every row of the store falls in ONE class:
  - each entry alone on a table that begin + insert have filled: the clearing of the counts, silo_gpu_distinct_count,
    silo_gpu_distinct_classes, silo_gpu_smallest_keys (k = 1 024 and 16 384);
  - the whole chain: begin, insert, the two memsets, count, classes, smallest_keys (k = 1 024);
  - the yardstick in the same run: begin, insert, select — what an `Aggregated` request under DistinctSequences runs.
--engine instead times requests through the engine on the same store (host clock, response text included): DistinctSequenceCounts
(default maxClasses, and 16 384) and `Aggregated` under DistinctSequences of the same child.
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
    """--engine: the host clock around whole requests, one engine, the first request under DistinctSequences (which computes the kept
    hashes) made before anything is timed."""
    from silo_amd.engine import Engine

    n = args.sequences
    genomes, _, tree, lineage, model = synthetic_model(n)
    children = {"True": {"type": "True"},
                f"PangoLineage {bench.QUERY_LINEAGE}*": {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}}
    engine = Engine(genomes)
    engine.set_schema("key", None)
    partition = engine.add_partition(n)
    engine.generate_synthetic(partition, "main", False, model, engine.position_window("main", False))
    engine.set_lineage_column_ids(partition, "pango_lineage", tree.names, lineage)
    engine.append_metadata(partition, "key", "string", [f"S{i}" for i in range(n)])
    engine.finalize()

    def request_ms(action, expression):
        """(median ms of --reps requests behind a warm-up, the last response's rows)"""
        request = json.dumps({"action": action, "filterExpression": expression}).encode()
        times = []
        for _ in range(args.reps + 1):
            t = time.perf_counter()
            status, body = engine.execute_text(request)
            times.append((time.perf_counter() - t) * 1e3)
            assert status == 200, body[:500]
        return round(float(np.median(times[1:])), 4), json.loads(body.decode())["queryResult"]

    for name, child in children.items():
        distinct = {"type": "DistinctSequences", "child": child}
        yardstick_ms, counted = request_ms({"type": "Aggregated"}, distinct)
        action_ms, rows = request_ms({"type": "DistinctSequenceCounts"}, child)
        most_ms, most_rows = request_ms({"type": "DistinctSequenceCounts", "maxClasses": 16384}, child)
        one_ms, _ = request_ms({"type": "DistinctSequenceCounts", "maxClasses": 1}, child)
        print(json.dumps({
            "sequences": n, "child": name, "distinct_rows": counted[0]["count"], "aggregated_under_distinct_ms": yardstick_ms,
            "distinct_sequence_counts_ms": action_ms, "rows": len(rows), "largest": rows[0], "ratio": round(action_ms / yardstick_ms, 3),
            "max_classes_16384_ms": most_ms, "rows_16384": len(most_rows), "max_classes_1_ms": one_ms,
        }), flush=True)
    engine.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--engine", action="store_true", help="time requests through the engine instead of the C entries")
    args = parser.parse_args()
    if args.engine:
        return through_the_engine(args)

    from silo_amd import binding

    lib = binding.load_library()
    n = args.sequences
    _, reference, tree, lineage, model = synthetic_model(n)
    member = tree.subtree(tree.names.index(bench.QUERY_LINEAGE)).astype(bool)

    def timed(launches, prepare=None):
        """Median of HIP event timings (ms) around `launches`, behind one warm-up run; `prepare` runs untimed ahead of each."""
        times = []
        for _ in range(args.reps + 1):
            if prepare is not None:
                prepare()
                binding._check(lib.silo_gpu_stream_synchronize(None))
            events = [binding.GpuEvent() for _ in range(2)]
            events[0].record()
            launches()
            events[1].record()
            binding._check(lib.silo_gpu_stream_synchronize(None))
            times.append(events[0].elapsed_ms(events[1]))
        return round(float(np.median(times[1:])), 4)

    with binding.GpuStore(n, [dict(name="main", alphabet="nuc", reference=reference)]) as store:
        store.generate_synthetic(0, model)
        store.finalize()
        row_words = store.row_words
        hashes = store.malloc(row_words * 64 * 16)
        scratch = store.malloc(binding.row_hash_scratch_bytes(len(reference)))
        binding._check(lib.silo_gpu_row_hashes(store.handle, 0, hashes, scratch, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        equal_hashes = binding.device_malloc(row_words * 64 * 16, 0x5A)  # every row the same hash: one class of all rows

        slots = binding.distinct_slots(n)
        table = binding.device_malloc(binding.distinct_table_bytes(slots))
        counts = binding.device_malloc(binding.distinct_counts_bytes(slots))
        keys = binding.device_malloc(n * 8)
        out_bitset = binding.device_malloc(row_words * 8)
        small = binding.device_malloc(binding.MAX_DISTINCT_CLASSES * 8 + 8)  # the selected keys, their number, the key counter
        out_count = ctypes.c_void_p(small.value + binding.MAX_DISTINCT_CLASSES * 8)
        n_keys = ctypes.c_void_p(small.value + binding.MAX_DISTINCT_CLASSES * 8 + 4)
        select_scratch = binding.device_malloc(binding.SMALLEST_KEYS_SCRATCH_BYTES)
        parts = {}
        for label, pointer in (("store", hashes), ("equal", equal_hashes)):
            record = np.zeros(1, dtype=binding.DISTINCT_PART_DTYPE)
            record[0] = (pointer.value, 0, n, row_words, 0)
            parts[label] = binding._upload(record)

        def measure(name, mask, which):
            filter_dev = binding._upload(words_of(mask, row_words))
            part = parts[which]

            def build():
                binding._check(lib.silo_gpu_distinct_begin(table, slots, None))
                binding._check(lib.silo_gpu_distinct_insert(table, slots, part, 1, 0, filter_dev, None))

            def clear():
                binding._check(lib.silo_gpu_memset_async(counts, 0, binding.distinct_counts_bytes(slots), None))
                binding._check(lib.silo_gpu_memset_async(n_keys, 0, 4, None))

            def count():
                binding._check(lib.silo_gpu_distinct_count(table, slots, counts, part, 1, 0, filter_dev, None))

            def classes():
                binding._check(lib.silo_gpu_distinct_classes(table, slots, counts, part, 1, 0, filter_dev, 1, keys, n, n_keys, None))

            def smallest(k):
                binding._check(lib.silo_gpu_smallest_keys(keys, n_keys, n, k, small, out_count, select_scratch, None))

            def chain():
                build()
                clear()
                count()
                classes()
                smallest(1024)

            def yardstick():
                build()
                binding._check(lib.silo_gpu_distinct_select(table, slots, part, 1, 0, filter_dev, out_bitset, None))

            chain_ms = timed(chain)
            yardstick_ms = timed(yardstick)
            build()
            clear_ms = timed(clear)
            count_ms = timed(count, prepare=clear)
            classes_ms = timed(classes, prepare=lambda: binding._check(lib.silo_gpu_memset_async(n_keys, 0, 4, None)))
            smallest_ms = {k: timed(lambda k=k: smallest(k)) for k in (1024, binding.MAX_DISTINCT_CLASSES)}
            n_classes = int(binding.device_read(n_keys, np.uint32, 1)[0])
            smallest(1)
            binding._check(lib.silo_gpu_stream_synchronize(None))
            largest = int(binding.device_read(small, np.uint64, 1)[0])
            overflow = int(binding.device_read(table, np.uint32, slots + 1)[-1])
            print(json.dumps({
                "sequences": n, "hashes": which, "filter": name, "filter_rows": int(mask.sum()), "slots": slots, "classes": n_classes, "overflow": overflow,
                "largest_class": 0xFFFFFFFF - (largest >> 32), "its_representative": largest & 0xFFFFFFFF,
                "clear_counts_ms": clear_ms, "count_ms": count_ms, "classes_ms": classes_ms, "smallest_keys_1024_ms": smallest_ms[1024],
                "smallest_keys_16384_ms": smallest_ms[binding.MAX_DISTINCT_CLASSES], "chain_ms": chain_ms, "begin_insert_select_ms": yardstick_ms,
                "ratio": round(chain_ms / yardstick_ms, 3),
            }), flush=True)
            binding.device_free(filter_dev)
            return largest & 0xFFFFFFFF

        everything = np.ones(n, dtype=bool)
        representative = measure("True", everything, "store")
        measure(f"PangoLineage {bench.QUERY_LINEAGE}*", member[lineage], "store")
        # the rows of the store's largest class: those whose hash is its representative's
        host_hashes = binding.device_read(hashes, np.uint64, n * 2).reshape(n, 2)
        measure("the largest class of the store", (host_hashes == host_hashes[representative]).all(axis=1), "store")
        measure("True", everything, "equal")
        for ptr in (table, counts, keys, out_bitset, small, select_scratch, equal_hashes, *parts.values()):
            binding.device_free(ptr)
        store.free(hashes)
        store.free(scratch)


if __name__ == "__main__":
    main()
