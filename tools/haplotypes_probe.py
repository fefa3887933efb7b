#!/usr/bin/env python3
"""Haplotypes probe (K16): on bench.py's synthetic genome store (--sequences rows), for --positions listed positions (default 1, 6
and 12, spread over the genome), under the filter True and under the largest lineage below the root (a PangoLineage filter with its
sublineages):
  - silo_gpu_position_symbols between HIP events;
  - silo_gpu_haplotype_ids and the count of its id columns under the filter — silo_gpu_group_count up to 2^20 potential tuples,
    silo_gpu_group_count_hashed beyond, the rule of the action — between HIP events;
  - what exists today for the same cells: positions x 16 calls of silo_gpu_store_sparse_plane, one (position, symbol) bitset each,
    between HIP events;
  - one Haplotypes request, host clock around a request that ends in a fetch the host waits for, response text included, not parsed.
Medians of --reps runs after one that warms up.  Prints one JSON line per (positions, filter); no ratio is asserted."""
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

N_SYMBOLS = 16
DENSE_HISTOGRAM_LIMIT = 1 << 20  # as the action's group-by takes the dense histogram


def listed_positions(k, positions):
    """k positions (0-based) spread over the genome, away from its ends, not in ascending order."""
    spread = [int((i + 1) * positions / (k + 1)) for i in range(k)]
    return spread[1::2] + spread[0::2]


def kernel_times(n_sequences, position_counts, reps):
    """(positions, filter) -> the medians on a store of bench's model; the lineage tree."""
    from silo_amd import alphabet, binding, synth

    genomes = bench.load_reference_genomes(False)
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in genomes["nucleotideSequences"][0]["sequence"]], dtype=np.uint8)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n_sequences, tree, synth.DEFAULT_SEED)
    model = synth.make_model(n_sequences, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    store = binding.GpuStore(n_sequences, [dict(name="main", alphabet="nuc", reference=reference)])
    store.generate_synthetic(0, model)
    store.finalize()
    lib = store.lib
    rows = store.row_words * 64
    lineage_filter = store.bitset_alloc()
    store.bitset_from_lineages(lineage_filter, tree.subtree(1))
    plane = store.bitset_alloc()
    out = {}
    for k in position_counts:
        listed = listed_positions(k, len(reference))
        n_columns = (k + binding.HAPLOTYPE_POSITIONS_PER_COLUMN - 1) // binding.HAPLOTYPE_POSITIONS_PER_COLUMN
        symbols = store.malloc(k * rows)
        unresolved = store.malloc(4)
        columns = [store.malloc(rows * 4) for _ in range(n_columns)]
        column_array = (ctypes.c_void_p * n_columns)(*[c.value for c in columns])
        cardinalities = [N_SYMBOLS ** min(binding.HAPLOTYPE_POSITIONS_PER_COLUMN, k - 6 * j) for j in range(n_columns)]
        cardinality_array = (ctypes.c_uint32 * n_columns)(*cardinalities)
        n_bins = int(np.prod(cardinalities, dtype=np.float64))
        dense = n_bins <= DENSE_HISTOGRAM_LIMIT
        counts = store.malloc(4 * n_bins) if dense else None
        symbols_ms = timed(reps, lambda: store.position_symbols_call(0, listed, symbols, unresolved))
        store.synchronize()
        assert int(store.read(unresolved, np.uint32, 1)[0]) == 0
        planes_ms = timed(reps, lambda: [store.sparse_plane(0, p, s, plane) for p in listed for s in range(N_SYMBOLS)])
        for name, filter_ptr in (("True", None), ("lineage", lineage_filter)):
            selected = n_sequences if filter_ptr is None else int(tree.subtree(1)[lineage].sum())
            groups = ctypes.c_uint32()

            def count():
                binding._check(lib.silo_gpu_haplotype_ids(symbols, k, store.row_words, n_sequences, N_SYMBOLS, binding.ALL_SYMBOLS_COMPLETE, filter_ptr,
                                                          column_array, None, None))
                if dense:
                    store.memset(counts, 0, 4 * n_bins)
                    binding._check(lib.silo_gpu_group_count(store.handle, filter_ptr, column_array, cardinality_array, n_columns, counts, None))
                else:
                    keys, tuple_counts = ctypes.c_void_p(), ctypes.c_void_p()
                    binding._check(lib.silo_gpu_group_count_hashed(store.handle, filter_ptr, column_array, cardinality_array, n_columns, selected,
                                                                   ctypes.byref(keys), ctypes.byref(tuple_counts), ctypes.byref(groups), None))
                    store.free(keys)
                    store.free(tuple_counts)

            count_ms = timed(reps, count)
            store.synchronize()
            out[k, name] = {"position_symbols_ms_median": symbols_ms, "ids_and_count_ms_median": count_ms, "count_path": "dense" if dense else "hashed",
                            "sparse_plane_calls": k * N_SYMBOLS, "sparse_planes_ms_median": planes_ms, "symbol_bytes": k * rows, "selected_rows": selected}
        for pointer in [symbols, unresolved, *columns] + ([counts] if dense else []):
            store.free(pointer)
    store.free(lineage_filter)
    store.free(plane)
    store.close()
    return out, tree


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--positions", type=int, nargs="+", default=[1, 6, 12])
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    kernels, tree = kernel_times(args.sequences, args.positions, args.reps)
    t0 = time.perf_counter()
    engine = build_engine(args.sequences)
    build_s = time.perf_counter() - t0
    print(f"store of {args.sequences} rows built in {build_s:.1f} s", file=sys.stderr, flush=True)
    genome_length = len(bench.load_reference_genomes(False)["nucleotideSequences"][0]["sequence"])
    filters = {"True": {"type": "True"},
               "lineage": {"type": "PangoLineage", "column": "pango_lineage", "value": tree.names[1], "includeSublineages": True}}
    for k in args.positions:
        listed = listed_positions(k, genome_length)
        for name, expression in filters.items():
            body = json.dumps({"action": {"type": "Haplotypes", "positions": [p + 1 for p in listed]}, "filterExpression": expression}).encode()
            request_ms = []
            text = b""
            for rep in range(args.reps + 1):  # the first request warms up
                t = time.perf_counter()
                status, text = engine.execute_text(body)
                elapsed = (time.perf_counter() - t) * 1e3
                assert status == 200, text[:500]
                if rep:
                    request_ms.append(elapsed)
            rows = json.loads(text.decode())["queryResult"]
            line = {"sequences": args.sequences, "positions": k, "filter": name, "build_s": round(build_s, 1), "haplotypes": len(rows),
                    "rows_counted": sum(row["count"] for row in rows), "request_ms": [round(x, 3) for x in request_ms],
                    "request_ms_median": round(float(np.median(request_ms)), 3), "response_bytes": len(text)}
            line.update(kernels[k, name])
            print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
