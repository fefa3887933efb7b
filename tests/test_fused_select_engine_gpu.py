"""Mutations queries whose scans are the only writers of their count table leave through silo_gpu_mutations_scan_select (no fill
launch, no selection launch; Mutations::begin, ScanBatcher::flush): the response bodies do not depend on whether the finish
kernel of the scan selects the rows (SILO_GPU_TUNE_FUSED_SELECT 0) or the call clears, scans and selects (-1) — in one partition,
in two partitions with both or one of them selected, with a row slot too small for the rows, and at minProportion 0."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TUNE_LAUNCH_COST, TUNE_FUSED_SELECT = 9, 13
PART_ROWS = 66_000  # a partition's stores are re-encoded from 65 536 rows on
STORES = (("main", False, 600, "ACGT", "N"), ("S", True, 120, "ACDEFGHIKLMNPQRSTVWY", "X"), ("ORF9", True, 97, "ACDEFGHIKLMNPQRSTVWY", "X"))


def engine_of(n_partitions):
    """The genome stub and two short genes, ragged at both ends, with runs of the missing symbol; lineages of a synthetic tree."""
    from silo_amd import synth
    from silo_amd.engine import Engine

    rng = np.random.default_rng(101)
    rows = PART_ROWS * n_partitions
    tree = synth.make_lineage_tree(40)
    lineage = synth.assign_lineages(rows, tree, 7)
    references, sequences = {}, {}
    for name, _, positions, letters, missing in STORES:
        alphabet = np.frombuffer(letters.encode(), dtype=np.uint8)
        reference_index = rng.integers(0, len(alphabet), size=positions)
        reference = alphabet[reference_index]
        second = alphabet[(reference_index + 1) % len(alphabet)]
        draw = rng.random((rows, positions), dtype=np.float32)
        chars = np.where(draw < 0.002, second, reference).astype(np.uint8)
        for p in (1, positions // 3, positions // 2, positions - 2):  # reported at 0.05, two of them inside the ragged ends
            chars[rng.random(rows) < 0.08, p] = second[p]
        lead = np.where(rng.random(rows) < 0.97, rng.geometric(1 / 20, size=rows), 0)
        trail = np.where(rng.random(rows) < 0.97, rng.geometric(1 / 40, size=rows), 0)
        column = np.arange(positions)
        chars[column[None, :] < lead[:, None]] = ord("-")
        chars[column[None, :] >= positions - trail[:, None]] = ord("-")
        for row in rng.choice(rows, size=300 * n_partitions, replace=False):
            start = int(rng.integers(0, positions))
            chars[row, start:start + int(rng.geometric(1 / 20))] = ord(missing)
        references[name] = bytes(reference).decode()
        sequences[name] = [bytes(row).decode() for row in chars]
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": references["main"]}],
                     "genes": [{"name": name, "sequence": references[name]} for name, is_aa, *_ in STORES if is_aa]})
    engine.set_schema("key", "date")
    for k in range(n_partitions):
        lo, hi = k * PART_ROWS, (k + 1) * PART_ROWS
        part = engine.add_partition(PART_ROWS)
        for name, is_aa, *_ in STORES:
            engine.append_sequences(part, name, is_aa, 0, sequences[name][lo:hi])
        engine.append_metadata(part, "key", "string", [str(i) for i in range(lo, hi)])
        engine.append_metadata(part, "date", "date", ["2021-03-04"] * PART_ROWS)
        engine.append_metadata(part, "part", "int", [str(k)] * PART_ROWS)
        engine.set_lineage_column_ids(part, "pango_lineage", tree.names, lineage[lo:hi])
    engine.finalize()
    counts = np.bincount(lineage, minlength=len(tree.names))
    frequent = [tree.names[i] for i in np.argsort(-counts)[:8]]
    return engine, frequent


def lineage_filter(name):
    return {"type": "PangoLineage", "column": "pango_lineage", "value": name, "includeSublineages": True}


@pytest.mark.parametrize("n_partitions", [1, 2])
def test_bodies_do_not_depend_on_where_the_rows_are_selected(built, n_partitions):
    from silo_amd import binding

    lib = binding.load_library()
    lib.silo_gpu_tune(TUNE_LAUNCH_COST, -1)
    try:
        engine, frequent = engine_of(n_partitions)
    finally:
        lib.silo_gpu_tune(TUNE_LAUNCH_COST, 0)
    for k in range(n_partitions):
        view = engine.partition_store(k)
        assert int(lib.silo_gpu_store_scan_runs(view.handle, engine.seqstore_id(k, "main", False))) > 0, k  # derived symbols
    filters = [lineage_filter(frequent[1])]  # (the most frequent one is the root: every row)
    if n_partitions == 2:  # ... and with one partition selected: the scans of the other drop out
        filters.append({"type": "And", "children": [lineage_filter(frequent[1]), {"type": "IntBetween", "column": "part", "from": 1, "to": 1}]})

    def run_all(proportion):
        bodies = []
        for expression in filters:
            for action in ({"type": "Mutations"}, {"type": "AminoAcidMutations"}, {"type": "Mutations", "sequenceNames": ["main"]},
                           {"type": "AminoAcidMutations", "sequenceNames": ["ORF9"]}):
                bodies.append(engine.execute_text(json.dumps({"action": dict(action, minProportion=proportion), "filterExpression": expression})))
        batch = [json.dumps({"action": {"type": "Mutations" if i % 2 == 0 else "AminoAcidMutations", "minProportion": proportion},
                             "filterExpression": lineage_filter(name)}) for i, name in enumerate(frequent)]
        bodies.extend(engine.execute_batch_text(batch))
        bodies.extend(engine.execute_batch_text([json.dumps({"action": {"type": "Mutations", "minProportion": proportion},
                                                             "filterExpression": lineage_filter(name)}) for name in frequent]))
        return bodies

    for capacity, proportion in ((4096, 0.05), (2, 0.05), (4096, 0.0)):
        engine.set_option("mutation_row_capacity", capacity)
        bodies = {}
        for value in (0, -1):
            previous = lib.silo_gpu_tune(TUNE_FUSED_SELECT, value)
            try:
                bodies[value] = run_all(proportion)
            finally:
                lib.silo_gpu_tune(TUNE_FUSED_SELECT, previous)
        assert all(status == 200 for status, _ in bodies[0]), [body for status, body in bodies[0] if status != 200][:1]
        assert bodies[0] == bodies[-1], (capacity, proportion)
        assert all(json.loads(body)["queryResult"] for _, body in bodies[0][:4]), (capacity, proportion)
        if capacity == 4096 and proportion == 0.05:
            reference = bodies[0]
        elif proportion == 0.05:
            assert bodies[0] == reference  # the fallback fetch of the whole table gives the same rows
    engine.set_option("mutation_row_capacity", 4096)
    engine.close()
