#!/usr/bin/env python3
"""Sample probe (K19), on the C entries alone: --sequences rows in one partition, the filter of all rows and the row set of
bench.py's lineage filter (QUERY_LINEAGE with sublineages, lineages assigned to rows as bench.py's store assigns them), without
strata and with --strata weekly date ranges (dates uniform over 60 weeks, so some rows fall in no range).  HIP events on the null
stream, median of --reps runs behind one warm-up each:
  - the whole selection: silo_gpu_sample_begin, four rounds of silo_gpu_sample_count + silo_gpu_sample_advance, silo_gpu_sample_select;
  - round 0's silo_gpu_sample_count alone (it touches every selected row; the later rounds 1/256 of them);
  - silo_gpu_sample_groups alone (with its table upload and its wait), which the selection above does not include;
  - silo_gpu_stream_read_probe over the bytes one pass reads (the bitset, plus 2 bytes per row of groups): what the same device
    needs to stream them once.  A selection makes five such passes (four counts and the select).
--engine instead times `Aggregated` requests through the engine on bench.py's synthetic genome store with such a date column.
Prints one JSON line per case; no ratio is asserted."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd")]

import bench  # noqa: E402


def words_of(mask, row_words):
    padded = np.zeros(row_words * 64, dtype=bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


def through_the_engine(args):
    """--engine: the host clock around `Aggregated` requests on bench.py's synthetic genome store with a date column (one
    partition): under the child alone, under Sample of it, and under Sample with the weekly ranges.  One JSON line per child."""
    import datetime
    import time

    from silo_amd import alphabet, synth
    from silo_amd.engine import Engine

    n = args.sequences
    genomes = bench.load_reference_genomes(False)
    reference = np.array([alphabet.NUCLEOTIDE.char_to_symbol[c] for c in genomes["nucleotideSequences"][0]["sequence"]], dtype=np.uint8)
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n, tree, synth.DEFAULT_SEED)
    model = synth.make_model(n, reference, "nuc", tree, lineage, seed=synth.DEFAULT_SEED, table_seed=synth.DEFAULT_SEED)
    first_day = datetime.date(2021, 1, 4)
    days = [str(first_day + datetime.timedelta(int(d))) for d in range(60 * 7)]
    offsets = np.random.default_rng(args.seed).integers(0, 60 * 7, size=n)
    engine = Engine(genomes)
    engine.set_schema("key", None)
    partition = engine.add_partition(n)
    engine.generate_synthetic(partition, "main", False, model, engine.position_window("main", False))
    engine.set_lineage_column_ids(partition, "pango_lineage", tree.names, lineage)
    engine.append_metadata(partition, "key", "string", [f"S{i}" for i in range(n)])
    engine.append_metadata(partition, "date", "date", [days[d] for d in offsets])
    engine.finalize()
    ranges = [{"dateFrom": days[7 * week], "dateTo": days[7 * week + 6]} for week in range(args.strata)]
    children = {"True": {"type": "True"},
                f"PangoLineage {bench.QUERY_LINEAGE}*": {"type": "PangoLineage", "column": "pango_lineage", "value": bench.QUERY_LINEAGE, "includeSublineages": True}}

    def median_ms(expression):
        request = json.dumps({"action": {"type": "Aggregated"}, "filterExpression": expression}).encode()
        times = []
        for _ in range(args.reps + 1):  # the first run warms up
            t = time.perf_counter()
            status, body = engine.execute_text(request)
            times.append((time.perf_counter() - t) * 1e3)
            assert status == 200, body[:500]
        return round(float(np.median(times[1:])), 4), json.loads(body.decode())["queryResult"][0]["count"]

    for name, child in children.items():
        sample = {"type": "Sample", "child": child, "size": args.size, "seed": args.seed}
        child_ms, child_count = median_ms(child)
        sample_ms, sample_count = median_ms(sample)
        strata_ms, strata_count = median_ms(dict(sample, dateField="date", dateRanges=ranges))
        print(json.dumps({
            "sequences": n, "child": name, "size": args.size, "strata": args.strata, "aggregated_under_child_ms": child_ms, "child_rows": child_count,
            "aggregated_under_sample_ms": sample_ms, "sample_rows": sample_count, "aggregated_under_sample_with_strata_ms": strata_ms,
            "sample_with_strata_rows": strata_count,
        }), flush=True)
    engine.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sequences", type=int, default=10_000_000)
    parser.add_argument("--size", type=int, default=2000)
    parser.add_argument("--strata", type=int, default=52)
    parser.add_argument("--seed", type=int, default=7)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--engine", action="store_true", help="time requests through the engine instead of the C entries")
    args = parser.parse_args()
    if args.engine:
        return through_the_engine(args)

    from silo_amd import binding, synth

    lib = binding.load_library()
    n = args.sequences
    row_words = (n + 2047) // 2048 * 32  # whole 256-byte lines, as a store lays its rows out
    tree = synth.make_lineage_tree(bench.N_LINEAGES)
    lineage = synth.assign_lineages(n, tree, synth.DEFAULT_SEED)
    member = tree.subtree(tree.names.index(bench.QUERY_LINEAGE)).astype(bool)
    rng = np.random.default_rng(args.seed)
    day0 = 18_000
    dates = np.zeros(row_words * 64, dtype=np.uint32)
    dates[:n] = day0 + rng.integers(0, 60 * 7, size=n)
    bounds = np.array([[day0 + 7 * week, day0 + 7 * week + 6] for week in range(args.strata)], dtype=np.uint32)
    filters = {"True": np.ones(n, dtype=bool), f"PangoLineage {bench.QUERY_LINEAGE}*": member[lineage]}

    dates_dev = binding._upload(dates)
    groups_dev = binding.device_malloc(row_words * 64 * 2)
    out_dev = binding.device_malloc(row_words * 8)

    def timed(launches):
        """Median of HIP event timings (ms) around `launches`, behind one warm-up run."""
        times = []
        for _ in range(args.reps + 1):
            events = [binding.GpuEvent() for _ in range(2)]
            events[0].record()
            launches()
            events[1].record()
            binding._check(lib.silo_gpu_stream_synchronize(None))
            times.append(events[0].elapsed_ms(events[1]))
        return round(float(np.median(times[1:])), 4)

    for name, mask in filters.items():
        filter_dev = binding._upload(words_of(mask, row_words))
        for n_groups, groups in ((1, None), (args.strata, groups_dev)):
            state = binding.device_malloc(binding.sample_state_bytes(n_groups))

            def make_groups():
                binding._check(lib.silo_gpu_sample_groups(filter_dev, dates_dev, binding._ptr(bounds), len(bounds), n, row_words, groups_dev, None))

            def round_zero():
                binding._check(lib.silo_gpu_sample_count(state, filter_dev, groups, n, row_words, 0, 0, None))

            def selection():
                binding._check(lib.silo_gpu_sample_begin(state, n_groups, args.size, args.seed, None))
                for sample_round in range(binding.SAMPLE_ROUNDS):
                    binding._check(lib.silo_gpu_sample_count(state, filter_dev, groups, n, row_words, 0, sample_round, None))
                    binding._check(lib.silo_gpu_sample_advance(state, sample_round, None))
                binding._check(lib.silo_gpu_sample_select(state, filter_dev, groups, n, row_words, 0, out_dev, None))

            groups_ms = timed(make_groups) if groups is not None else None
            selection_ms = timed(selection)
            selected = int(np.unpackbits(binding.device_read(out_dev, np.uint8, row_words * 8)).sum())
            binding._check(lib.silo_gpu_sample_begin(state, n_groups, args.size, args.seed, None))
            round_zero_ms = timed(round_zero)
            pass_bytes = row_words * 8 + (row_words * 64 * 2 if groups is not None else 0)
            read_ms = ctypes.c_float()
            binding._check(lib.silo_gpu_stream_read_probe(pass_bytes, 50, ctypes.byref(read_ms)))
            print(json.dumps({
                "sequences": n, "filter": name, "filter_rows": int(mask.sum()), "strata": 0 if groups is None else args.strata, "size": args.size,
                "selected_rows": selected, "selection_ms": selection_ms, "round_0_count_ms": round_zero_ms, "sample_groups_ms": groups_ms,
                "bytes_per_pass": pass_bytes, "stream_read_of_one_pass_ms": round(read_ms.value, 4), "passes": binding.SAMPLE_ROUNDS + 1,
            }), flush=True)
            binding.device_free(state)
        binding.device_free(filter_dev)
    for ptr in (dates_dev, groups_dev, out_dev):
        binding.device_free(ptr)


if __name__ == "__main__":
    main()
