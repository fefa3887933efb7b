#!/usr/bin/env python3
"""MutationsPerSequence probe (K18): on bench.py's synthetic genome store (--sequences rows), for --rows selected rows (default 100,
1 000 and 10 000: a stretch of consecutive rows a third into the store):
  - silo_gpu_reconstruct_sequences of the rows into one [n x positions] buffer and silo_gpu_sequence_differences over it with room
    for 32 x n words, each between HIP events, medians of --reps runs after one that warms up, with K18's bytes — the characters read
    twice (count pass, write pass), the reference, the per-chunk counts, the offsets, stats and words written — over its time;
  - one MutationsPerSequence request for the rows, and what a client needs today for them: one FastaAligned request (unchanged code,
    the same build; the client's own comparison of the strings is NOT in the time); host clock around a request that ends in a
    fetch the host waits for, response text included, not parsed, the two alternated.
Prints one JSON line per selection; no ratio is asserted."""
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

WORDS_PER_ROW = 32  # MutationsPerSequence::FIRST_WORDS_PER_ROW: the words per row the first call of a request has room for


def kernel_times(n_sequences, selections, reps):
    """Per selection size the medians of the gather and of K18 on a store of bench's model, and K18's counts and bytes."""
    from silo_amd import alphabet, binding, synth

    genomes = bench.load_reference_genomes(False)
    text = genomes["nucleotideSequences"][0]["sequence"]
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in text], dtype=np.uint8)
    positions = len(reference)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n_sequences, tree, synth.DEFAULT_SEED)
    model = synth.make_model(n_sequences, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    store = binding.GpuStore(n_sequences, [dict(name="main", alphabet="nuc", reference=reference)])
    store.generate_synthetic(0, model)
    store.finalize()
    lib = store.lib
    reference_chars = np.frombuffer(text.encode(), dtype=np.uint8)
    reference_dev = binding.device_malloc(positions)
    binding._check(lib.silo_gpu_memcpy_h2d(reference_dev, reference_chars.ctypes.data_as(ctypes.c_void_p), positions, None))
    out = {}
    for n in selections:
        rows = np.arange(n_sequences // 3, n_sequences // 3 + n, dtype=np.uint32)
        rows_dev = store.upload_column(rows)
        capacity = WORDS_PER_ROW * n
        chars_dev = binding.device_malloc(n * positions)
        heads_dev = binding.device_malloc((n + 1 + n * binding.DIFFERENCE_STATS) * 4)
        records_dev = binding.device_malloc(capacity * 4)
        scratch_bytes = binding.differences_scratch_bytes(n, positions)
        scratch_dev = binding.device_malloc(scratch_bytes)
        stats_dev = ctypes.c_void_p(heads_dev.value + (n + 1) * 4)
        gather_ms = timed(reps, lambda: binding._check(lib.silo_gpu_reconstruct_sequences(store.handle, 0, rows_dev, n, chars_dev, None)))
        differences_ms = timed(reps, lambda: binding._check(
            lib.silo_gpu_sequence_differences(0, chars_dev, n, positions, reference_dev, capacity, heads_dev, stats_dev, records_dev, scratch_dev, None)))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        heads = binding.device_read(heads_dev, np.uint32, n + 1 + n * binding.DIFFERENCE_STATS)
        total = int(heads[n])
        written = min(total, capacity)
        # both passes read the characters and the reference; the count pass writes and the two small passes read the per-chunk words
        differences_bytes = 2 * (n * positions + positions) + 2 * scratch_bytes + len(heads) * 4 + written * 4
        out[n] = {
            "positions": positions, "gather_ms_median": gather_ms, "differences_ms_median": differences_ms, "differences_bytes": differences_bytes,
            "differences_gb_per_s": round(differences_bytes / differences_ms / 1e6, 1), "words": total, "first_capacity": capacity,
            "cells": heads[n + 1:].reshape(n, binding.DIFFERENCE_STATS).sum(axis=0).tolist(),
        }
        for pointer in (chars_dev, heads_dev, records_dev, scratch_dev):
            binding.device_free(pointer)
        store.free(rows_dev)
    binding.device_free(reference_dev)
    store.close()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=1_000_000)
    parser.add_argument("--rows", type=int, nargs="+", default=[100, 1000, 10000], help="selected sequences; one measurement each")
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()

    kernels = kernel_times(args.sequences, args.rows, args.reps)
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

    for n in args.rows:
        first = args.sequences // 3
        selection = {"type": "IntBetween", "column": "row", "from": first, "to": first + n - 1}
        per_sequence = json.dumps({"action": {"type": "MutationsPerSequence"}, "filterExpression": selection}).encode()
        fasta = json.dumps({"action": {"type": "FastaAligned", "sequenceName": "main"}, "filterExpression": selection}).encode()
        per_sequence_ms, fasta_ms, sizes = [], [], {}
        for rep in range(args.reps + 1):  # the first round warms up; alternated, so that drift hits both
            one, text = run(per_sequence)
            sizes["mutations_per_sequence_response_bytes"] = len(text)
            assert text.count(b'"substitutionCount":') == n
            other, text = run(fasta)
            sizes["fasta_aligned_response_bytes"] = len(text)
            if rep:
                per_sequence_ms.append(one)
                fasta_ms.append(other)
        line = {"sequences": args.sequences, "selected": n, "build_s": round(build_s, 1),
                "mutations_per_sequence_ms": [round(x, 3) for x in per_sequence_ms], "mutations_per_sequence_ms_median": round(float(np.median(per_sequence_ms)), 3),
                "fasta_aligned_ms": [round(x, 3) for x in fasta_ms], "fasta_aligned_ms_median": round(float(np.median(fasta_ms)), 3)}
        line.update(sizes)
        line.update(kernels[n])
        print(json.dumps(line), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
