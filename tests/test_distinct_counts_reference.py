"""The numpy statement of DistinctSequenceCounts (tests/distinct_counts_reference.py): the classes by hash against the classes by
exact equality on every symbol matrix the GPU tests of the action use, the key packing at hand-written pairs, and the constants of
the binding against the header.  Runs anywhere."""
import os
import re

import numpy as np

from tests import distinct_counts_reference as counts_ref
from tests import distinct_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixtures():
    from tests import test_distinct_gpu
    from tests.test_distance_matrix_gpu import N_ROWS
    from tests.test_mutations_over_time_gpu import _synthetic_matrix

    yield "planted main", test_distinct_gpu.planted_symbols(None)
    yield "planted S", test_distinct_gpu.planted_symbols("S")
    synthetic = _synthetic_matrix(np.random.default_rng(2026))  # the matrix of the fixture `synthetic` of tests/test_distance_matrix_gpu.py
    assert synthetic.shape[0] == N_ROWS
    yield "synthetic", synthetic


def test_classes_by_hash_are_the_classes_by_equality():
    rng = np.random.default_rng(3)
    seen = 0
    for name, sym in _fixtures():
        n = len(sym)
        hashes = ref.row_hashes(sym)
        for selected in (np.ones(n, dtype=bool), rng.random(n) < 0.5, np.arange(n) >= n // 3, np.zeros(n, dtype=bool)):
            by_hash = counts_ref.classes_by_hash(hashes, selected)
            assert by_hash == counts_ref.classes_by_equality(sym, selected), name
            assert sum(by_hash.values()) == int(selected.sum()), name
            assert sorted(by_hash) == np.flatnonzero(ref.select_by_hash(hashes, selected)).tolist(), name
        seen += 1
    assert seen == 3


def test_known_classes():
    sym = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 4], [3, 2, 1], [1, 2, 3], [1, 2, 4]])
    assert counts_ref.classes(sym, [1, 1, 1, 1, 1, 1]) == {0: 3, 2: 2, 3: 1}
    assert counts_ref.classes(sym, [0, 1, 0, 1, 1, 1]) == {1: 2, 3: 1, 5: 1}
    assert counts_ref.classes(sym, [0, 0, 0, 0, 0, 0]) == {}
    assert counts_ref.classes_by_hash(ref.row_hashes(sym), [1, 1, 1, 1, 1, 1], first_row=10) == {10: 3, 12: 2, 13: 1}
    everything = counts_ref.classes(sym, [1, 1, 1, 1, 1, 1])
    assert counts_ref.unpack(counts_ref.packed_keys(everything)) == [(3, 0), (2, 2), (1, 3)]
    assert counts_ref.unpack(counts_ref.packed_keys(everything, min_count=2)) == [(3, 0), (2, 2)]
    assert counts_ref.unpack(counts_ref.first_keys(everything, 1)) == [(3, 0)]
    assert len(counts_ref.first_keys(everything, 5, min_count=4)) == 0


def test_the_key_packing():
    from silo_amd import binding

    for (count, row), want in (((1, 0), 0xFFFFFFFE00000000), ((4, 3), 0xFFFFFFFB00000003), ((0xFFFFFFFE, 0xFFFFFFFD), 0x00000001FFFFFFFD)):
        assert counts_ref.key(count, row) == want == binding.distinct_class_key(count, row)
        assert counts_ref.unpack([want]) == [(count, row)]
    # ascending keys: descending counts, then ascending rows
    assert counts_ref.key(5, 9) < counts_ref.key(4, 0) < counts_ref.key(4, 1) < counts_ref.key(1, 0)


def test_the_constants_of_the_binding_are_the_headers():
    from silo_amd import binding

    header = open(os.path.join(ROOT, "include", "silo_gpu.h")).read()
    assert int(re.search(r"#define SILO_GPU_MAX_DISTINCT_CLASSES (\d+)", header).group(1)) == binding.MAX_DISTINCT_CLASSES == 16384
    assert int(re.search(r"#define SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES (\d+)u", header).group(1)) == binding.SMALLEST_KEYS_SCRATCH_BYTES
    assert "#define SILO_GPU_DISTINCT_COUNTS_BYTES(slots) ((size_t)(slots) * 4u)" in header
    assert binding.distinct_counts_bytes(1 << 20) == 4 << 20
    for name in ("silo_gpu_distinct_count", "silo_gpu_distinct_classes", "silo_gpu_smallest_keys"):
        assert name in binding.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", header)
