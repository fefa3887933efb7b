#!/usr/bin/env python3
"""Consensus probe (K15): on bench.py's synthetic genome store (--sequences rows), for --groups lineage groups (default 1, 8 and 64:
subtrees of the lineage tree, as PangoLineage filters with their sublineages):
  - silo_gpu_mutations_scan_batch of the groups' bitsets into one table per group and silo_gpu_consensus_call over those tables,
    each between HIP events, medians of --reps runs after one that warms up (the tables are cleared before every scan, outside the
    events), with K15's bytes — the tables and the reference index read, the characters and the sums written — over its time;
  - one Consensus request of the groups, and what a client sends today for the same groups: one Mutations{minProportion: 0.5}
    request per group (the whole set where --mutations-all allows, 64 by default), host clock around a request that ends in a
    fetch the host waits for, response text included, not parsed, the two alternated.
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
from distance_probe import build_engine  # noqa: E402

N_SYMBOLS = 5


def lineage_roots(tree, n_groups):
    """The first n_groups lineages below the root (which is every row): subtrees from a third of the rows down to about a hundredth."""
    assert n_groups < len(tree.names)
    return list(range(1, n_groups + 1))


def kernel_times(n_sequences, group_counts, reps, threshold, min_depth):
    """(per group count the medians of the batched scan and of K15 on a store of bench's model and K15's bytes, the lineage tree)"""
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
        chars_dev = binding.device_malloc(q * positions)
        summary_dev = binding.device_malloc(q * 16)
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
        call_ms = timed(reps, lambda: binding._check(
            lib.silo_gpu_consensus_call(0, tables_dev, q, positions, reference_dev, threshold, min_depth, chars_dev, summary_dev, None)))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        summary = binding.device_read(summary_dev, np.uint32, q * 4).reshape(q, 4)
        call_bytes = table_bytes + q * positions + q * positions + q * 16  # tables, the reference index per table, characters, sums
        out[q] = {
            "scan_batch_ms_median": round(float(np.median(scan_ms[1:])), 4), "consensus_call_ms_median": call_ms, "consensus_call_bytes": call_bytes,
            "consensus_call_gb_per_s": round(call_bytes / call_ms / 1e6, 1), "ambiguous_positions": int(summary[:, 0].sum()),
            "low_coverage_positions": int(summary[:, 1].sum()), "positions": positions,
        }
        for pointer in (tables_dev, chars_dev, summary_dev):
            binding.device_free(pointer)
        for pointer in filters:
            store.free(pointer)
    binding.device_free(reference_dev)
    store.close()
    return out, tree


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--groups", type=int, nargs="+", default=[1, 8, 64])
    parser.add_argument("--threshold", type=float, default=0.5)
    parser.add_argument("--min-depth", type=int, default=1)
    parser.add_argument("--mutations-all", type=int, default=64, help="groups up to which every Mutations request is made")
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    kernels, tree = kernel_times(args.sequences, args.groups, args.reps, args.threshold, args.min_depth)
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
        consensus = json.dumps({"action": {"type": "Consensus", "groups": groups, "threshold": args.threshold, "minDepth": args.min_depth},
                                "filterExpression": {"type": "True"}}).encode()
        mutations = [json.dumps({"action": {"type": "Mutations", "sequenceName": "main", "minProportion": 0.5}, "filterExpression": expression}).encode()
                     for expression in expressions[:args.mutations_all]]
        consensus_ms, mutations_ms, sizes = [], [], {}
        for rep in range(args.reps + 1):  # the first round warms up; alternated, so that drift hits both
            elapsed, text = run(consensus)
            sizes["consensus_response_bytes"] = len(text)
            t = time.perf_counter()
            answers = [run(body)[1] for body in mutations]
            total = (time.perf_counter() - t) * 1e3
            sizes["mutations_response_bytes"] = sum(len(answer) for answer in answers)
            if rep:
                consensus_ms.append(elapsed)
                mutations_ms.append(total)
        rows = json.loads(run(consensus)[1].decode())["queryResult"]
        line = {"sequences": args.sequences, "groups": q, "threshold": args.threshold, "min_depth": args.min_depth, "build_s": round(build_s, 1),
                "group_rows": [row["count"] for row in rows][:8], "consensus_ms": [round(x, 3) for x in consensus_ms],
                "consensus_ms_median": round(float(np.median(consensus_ms)), 3), "mutations_requests_made": len(mutations),
                "mutations_all_groups_ms_median": round(float(np.median(mutations_ms)), 3) if len(mutations) == q else "not measured"}
        line.update(sizes)
        line.update(kernels[q])
        print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
