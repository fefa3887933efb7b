#!/usr/bin/env python3
"""MeanDistances probe (K24): on bench.py's synthetic genome store (--sequences rows, as tools/comparison_probe.py builds it), for
--groups lineage groups (default 1, 8 and 64: the first lineages below the root, as PangoLineage filters with their sublineages):
  - silo_gpu_mutations_scan_batch of the groups' bitsets into one table per group (the exact scan), between HIP events;
  - silo_gpu_table_pair_sums over those tables between HIP events, for the whole genome as one range and for the 98 tiling regions of
    400 positions of tools/region_counts_probe.py (an amplicon scheme: neighbours overlap), with the bytes the kernel stages — per tile
    of pairs the slabs of its tables — over its time;
  - silo_gpu_mutations_compare on the same tables in the same run (2 or more groups: K17 takes no single table);
  - one MeanDistances request of the groups, whole genome and the 98 regions: host clock around a request that ends in a fetch the host
    waits for, response text included, not parsed.
Medians of --reps runs after one that warms up.  Prints one JSON line per group count; no ratio is asserted."""
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
from region_counts_probe import tiling  # noqa: E402

CAPACITY = 1024  # of the comparison timed beside the sums
REGIONS = 98


def kernel_times(n_sequences, group_counts, reps):
    """(per group count the medians of the batched scan, of K24 over the genome and over the regions and of K17 on a store of bench's
    model, the lineage tree)"""
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
    genome = np.array([[0, positions]], dtype=np.uint32)
    regions = np.array(tiling(positions), dtype=np.uint32)
    out = {}
    for q in group_counts:
        filters = []
        for root in lineage_roots(tree, q):
            pointer = store.bitset_alloc()
            store.bitset_from_lineages(pointer, tree.subtree(root))
            filters.append(pointer)
        table_bytes = q * positions * N_SYMBOLS * 4
        tables_dev = binding.device_malloc(table_bytes)
        pairs = q * (q + 1) // 2
        sums_dev = binding.device_malloc(REGIONS * pairs * binding.PAIR_SUM_WORDS * 8)
        compare_dev = binding.device_malloc((binding.COMPARE_HEADER_WORDS + CAPACITY * 2 + CAPACITY * q * 2) * 4)
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

        def sums(ranges):
            return timed(reps, lambda: binding._check(
                lib.silo_gpu_table_pair_sums(0, tables_dev, q, positions, ranges.ctypes.data_as(ctypes.c_void_p), len(ranges), sums_dev, None)))

        genome_ms, regions_ms = sums(genome), sums(regions)
        compare_ms = None
        if q >= 2:
            compare_ms = timed(reps, lambda: binding._check(
                lib.silo_gpu_mutations_compare(0, tables_dev, q, positions, reference_dev, 0.05, 0.0, CAPACITY, compare_dev, None)))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        sides = (q + binding.PAIR_SUM_TILE - 1) // binding.PAIR_SUM_TILE
        # a tile of pairs off the diagonal stages two sets of up to 16 tables, one on it a single set: sides^2 sets in all
        genome_bytes = sides * q * positions * N_SYMBOLS * 4
        out[q] = {
            "scan_batch_ms_median": round(float(np.median(scan_ms[1:])), 4), "pair_sums_genome_ms_median": genome_ms,
            "pair_sums_98_regions_ms_median": regions_ms, "pair_sums_genome_bytes_staged": genome_bytes,
            "pair_sums_genome_gb_per_s": round(genome_bytes / genome_ms / 1e6, 1), "compare_ms_median": compare_ms, "positions": positions,
        }
        for pointer in (tables_dev, sums_dev, compare_dev):
            binding.device_free(pointer)
        for pointer in filters:
            store.free(pointer)
    binding.device_free(reference_dev)
    store.close()
    return out, tree, positions


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--groups", type=int, nargs="+", default=[1, 8, 64])
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    kernels, tree, positions = kernel_times(args.sequences, args.groups, args.reps)
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

    regions = [{"name": f"w{r}", "positionFrom": first + 1, "positionTo": end} for r, (first, end) in enumerate(tiling(positions))]
    for q in args.groups:
        names = [tree.names[root] for root in lineage_roots(tree, q)]
        groups = [{"name": name, "filterExpression": {"type": "PangoLineage", "column": "pango_lineage", "value": name, "includeSublineages": True}} for name in names]
        genome = json.dumps({"action": {"type": "MeanDistances", "groups": groups}, "filterExpression": {"type": "True"}}).encode()
        tiled = json.dumps({"action": {"type": "MeanDistances", "groups": groups, "regions": regions, "between": q <= 8}, "filterExpression": {"type": "True"}}).encode()
        genome_ms, tiled_ms, sizes = [], [], {}
        for rep in range(args.reps + 1):  # the first round warms up; alternated, so that drift hits both
            first, text = run(genome)
            sizes["genome_response_bytes"] = len(text)
            second, text = run(tiled)
            sizes["regions_response_bytes"] = len(text)
            if rep:
                genome_ms.append(first)
                tiled_ms.append(second)
        line = {"sequences": args.sequences, "groups": q, "build_s": round(build_s, 1), "request_genome_ms": [round(x, 3) for x in genome_ms],
                "request_genome_ms_median": round(float(np.median(genome_ms)), 3), "request_98_regions_ms_median": round(float(np.median(tiled_ms)), 3),
                "regions_between": q <= 8}  # 98 regions x 2 080 pairs of 64 groups are more than a response holds: within the groups only
        line.update(sizes)
        line.update(kernels[q])
        print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
