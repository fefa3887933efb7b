#!/usr/bin/env python3
"""MutationsComparison probe (K17): on bench.py's synthetic genome store (--sequences rows), for --groups lineage groups (default 2, 8
and 64: the first lineages below the root, as PangoLineage filters with their sublineages):
  - silo_gpu_mutations_scan_batch of the groups' bitsets into one table per group and silo_gpu_mutations_compare over those tables at
    (--min-proportion, 0), each between HIP events, medians of --reps runs after one that warms up (the tables are cleared before every
    scan, outside the events), with K17's bytes — the tables read once, the reference index, the records and their cells written —
    over its time;
  - one MutationsComparison request of the groups at (--min-proportion, 0) and at (--min-proportion, --min-difference), and what a
    correct client-side join needs today for the same groups: one Mutations{minProportion: 0} request per group, one after the other;
    host clock around a request that ends in a fetch the host waits for, response text included, not parsed, the three alternated.
Prints one JSON line per group count; no ratio is asserted."""
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
from clusters_probe import timed  # noqa: E402
from consensus_probe import N_SYMBOLS, lineage_roots  # noqa: E402
from distance_probe import build_engine  # noqa: E402

CAPACITY = 1024  # MutationsComparison::FIRST_CAPACITY: the records the first comparison of a request has room for


def kernel_times(n_sequences, group_counts, reps, min_proportion):
    """(per group count the medians of the batched scan and of K17 on a store of bench's model and K17's bytes, the lineage tree)"""
    from silo_amd import alphabet, binding, synth

    genomes = bench.load_reference_genomes(False)
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in genomes["nucleotideSequences"][0]["sequence"]], dtype=np.uint8)
    positions = len(reference)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n_sequences, tree, synth.DEFAULT_SEED)
    model = synth.make_model(n_sequences, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    store = binding.GpuStore(n_sequences, [dict(name="main", alphabet="nuc", reference=reference)])
    store.generate_synthetic(0, model)
    store.finalize()
    lib = store.lib
    reference_index = np.where(reference < N_SYMBOLS, reference, 0xFF).astype(np.uint8)  # "-ACGT" are the symbols 0 .. 4
    reference_dev = binding.device_malloc(positions)
    binding._check(lib.silo_gpu_memcpy_h2d(reference_dev, reference_index.ctypes.data_as(ctypes.c_void_p), positions, None))
    out = {}
    for q in group_counts:
        filters = []
        for root in lineage_roots(tree, q):
            pointer = store.bitset_alloc()
            store.bitset_from_lineages(pointer, tree.subtree(root))
            filters.append(pointer)
        table_bytes = q * positions * N_SYMBOLS * 4
        tables_dev = binding.device_malloc(table_bytes)
        out_words = binding.COMPARE_HEADER_WORDS + CAPACITY * 2 + CAPACITY * q * 2
        out_dev = binding.device_malloc(out_words * 4)
        filter_array = (ctypes.c_void_p * q)(*[f.value for f in filters])
        table_array = (ctypes.c_void_p * q)(*[tables_dev.value + t * positions * N_SYMBOLS * 4 for t in range(q)])
        scan_ms = []
        for _ in range(reps + 1):  # the first run warms up
            binding._check(lib.silo_gpu_memset_async(tables_dev, 0, table_bytes, None))
            begin, end = binding.GpuEvent(), binding.GpuEvent()
            begin.record()
            binding._check(lib.silo_gpu_mutations_scan_batch(store.handle, 0, filter_array, q, 0, positions, table_array, None))
            end.record()
            scan_ms.append(begin.elapsed_ms(end))
        compare_ms = timed(reps, lambda: binding._check(
            lib.silo_gpu_mutations_compare(0, tables_dev, q, positions, reference_dev, min_proportion, 0.0, CAPACITY, out_dev, None)))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        selected = int(binding.device_read(out_dev, np.uint32, 1)[0])
        written = min(selected, CAPACITY)
        compare_bytes = table_bytes + positions + 16 + written * 8 + written * q * 8  # tables, reference index, header, records, cells
        out[q] = {
            "scan_batch_ms_median": round(float(np.median(scan_ms[1:])), 4), "compare_ms_median": compare_ms, "compare_bytes": compare_bytes,
            "compare_gb_per_s": round(compare_bytes / compare_ms / 1e6, 1), "compare_selected": selected, "positions": positions,
        }
        for pointer in (tables_dev, out_dev):
            binding.device_free(pointer)
        for pointer in filters:
            store.free(pointer)
    binding.device_free(reference_dev)
    store.close()
    return out, tree


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--groups", type=int, nargs="+", default=[2, 8, 64])
    parser.add_argument("--min-proportion", type=float, default=0.05)
    parser.add_argument("--min-difference", type=float, default=0.5)
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    kernels, tree = kernel_times(args.sequences, args.groups, args.reps, args.min_proportion)
    t0 = time.perf_counter()
    engine = build_engine(args.sequences)
    build_s = time.perf_counter() - t0
    print(f"store of {args.sequences} rows built in {build_s:.1f} s", file=sys.stderr, flush=True)

    def run(body):
        t = time.perf_counter()
        status, text = engine.execute_text(body)
        elapsed = (time.perf_counter() - t) * 1e3
        assert status == 200, text[:500]
        return elapsed, text

    for q in args.groups:
        names = [tree.names[root] for root in lineage_roots(tree, q)]
        expressions = [{"type": "PangoLineage", "column": "pango_lineage", "value": name, "includeSublineages": True} for name in names]
        groups = [{"name": name, "filterExpression": expression} for name, expression in zip(names, expressions)]

        def comparison(min_difference):
            return json.dumps({"action": {"type": "MutationsComparison", "groups": groups, "minProportion": args.min_proportion, "minDifference": min_difference},
                               "filterExpression": {"type": "True"}}).encode()

        every, differing = comparison(0.0), comparison(args.min_difference)
        mutations = [json.dumps({"action": {"type": "Mutations", "sequenceName": "main", "minProportion": 0}, "filterExpression": expression}).encode()
                     for expression in expressions]
        every_ms, differing_ms, mutations_ms, sizes = [], [], [], {}
        for rep in range(args.reps + 1):  # the first round warms up; alternated, so that drift hits all three
            first, text = run(every)
            sizes["comparison_response_bytes"] = len(text)
            second, text = run(differing)
            sizes["comparison_min_difference_response_bytes"] = len(text)
            t = time.perf_counter()
            answers = [run(body)[1] for body in mutations]
            total = (time.perf_counter() - t) * 1e3
            sizes["mutations_response_bytes"] = sum(len(answer) for answer in answers)
            if rep:
                every_ms.append(first)
                differing_ms.append(second)
                mutations_ms.append(total)
        line = {"sequences": args.sequences, "groups": q, "min_proportion": args.min_proportion, "min_difference": args.min_difference, "build_s": round(build_s, 1),
                "comparison_ms": [round(x, 3) for x in every_ms], "comparison_ms_median": round(float(np.median(every_ms)), 3),
                "comparison_min_difference_ms_median": round(float(np.median(differing_ms)), 3),
                "mutations_all_groups_ms_median": round(float(np.median(mutations_ms)), 3)}
        line.update(sizes)
        line.update(kernels[q])
        print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
