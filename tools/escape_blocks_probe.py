"""The headline Mutations query under SILO_GPU_TUNE_ESCAPE_BLOCKS values in turn, inside ONE process (one database): per leg the
step of bench.py (20 steps after 3 warm-up steps) and, from one more query under the timing log, the escape launch's grid, items
and duration.  Usage: escape_blocks_probe.py [--sequences N] [--knobs 0,-1,0,-1,0,-1]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lapis-silo_amd")]
import bench  # noqa: E402
from silo_amd import binding  # noqa: E402

TUNE_SCAN_TIMING, TUNE_ESCAPE_BLOCKS = 7, 14

ap = argparse.ArgumentParser()
ap.add_argument("--sequences", type=int, default=10_000_000)
ap.add_argument("--knobs", type=str, default="0,-1,0,-1,0,-1", help="0 one block per item, -1 resident blocks, n > 0 exactly n blocks")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

lib = binding.load_library()
engine, model, tree, lineage, window = bench.build_engine(args.sequences, 0, 1, None, 0, with_genes=True)
query = bench.make_query()


def sync():
    binding._check(lib.silo_gpu_stream_synchronize(None))


found = lib.silo_gpu_tune(TUNE_ESCAPE_BLOCKS, 0)
for knob in [int(v) for v in args.knobs.split(",")]:
    lib.silo_gpu_tune(TUNE_ESCAPE_BLOCKS, knob)
    elapsed, rows = bench.run_steps(engine, query, args.steps, args.warmup, sync)
    lib.silo_gpu_tune(TUNE_SCAN_TIMING, 1)
    try:
        engine.execute_text(query.encode())
        launches = [entry for entry in binding.scan_timings() if entry["kernel"].startswith("k_scan_escapes_sliced<")]
    finally:
        lib.silo_gpu_tune(TUNE_SCAN_TIMING, 0)
    print(json.dumps({"knob": knob, "ms_per_step": elapsed / args.steps * 1e3, "rows": len(rows), "items": int(lib.silo_gpu_last_escape_items()),
                      "escape_launches": [{"kernel": e["kernel"], "blocks": e["blocks"], "us": e["ms"] * 1e3} for e in launches]}), flush=True)
lib.silo_gpu_tune(TUNE_ESCAPE_BLOCKS, found)
