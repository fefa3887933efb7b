"""tests/neighbours_reference.py (the numpy reference of K14) against a plain character double loop, the off-diagonal block of
tests/clusters_reference.pair_counts on the stacked rows and a full lexsort per row, and the constants of K14 that
silo_amd/binding.py restates against include/silo_gpu.h; runs without a GPU."""
import os
import re

import numpy as np
import pytest

from tests.clusters_reference import pair_counts
from tests.neighbours_reference import COLUMN_BITS, MAX_COLUMNS, MAX_NEIGHBOURS, MAX_ROWS, NOT_ELIGIBLE, cells_of, cross_counts, nearest_among, nearest_columns
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}


def _draw(rng, name, n, positions, changed=0.2):
    all_chars, valid_chars = ALPHABETS[name]
    base = rng.choice(np.frombuffer(valid_chars.encode(), dtype=np.uint8), size=positions)
    chars = np.tile(base, (n, 1))
    redrawn = rng.random((n, positions)) < changed
    chars[redrawn] = rng.choice(np.frombuffer(all_chars.encode(), dtype=np.uint8), size=int(redrawn.sum()))
    return chars


def _double_loop(chars_a, chars_b, valid_chars):
    differing = np.zeros((len(chars_a), len(chars_b)), dtype=np.uint32)
    compared = np.zeros_like(differing)
    valid = set(valid_chars.encode())
    for i, a in enumerate(chars_a.tolist()):
        for j, b in enumerate(chars_b.tolist()):
            for x, y in zip(a, b):
                if x in valid and y in valid:
                    compared[i, j] += 1
                    differing[i, j] += x != y
    return differing, compared


@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("m,n,positions", [(1, 1, 1), (3, 7, 63), (5, 4, 64), (9, 13, 65), (6, 20, 200), (4, 0, 9), (0, 4, 9), (3, 5, 0)])
def test_cross_counts_match_a_character_double_loop(name, m, n, positions):
    rng = np.random.default_rng(500 + m + 10 * n + positions)
    chars_a, chars_b = _draw(rng, name, m, positions), _draw(rng, name, n, positions)
    if positions > 2 and m and n:
        chars_a[0, :3] = [ord("a"), ord("?"), 0]  # bytes that are no symbol at all
        chars_b[0, :3] = [ord("a"), ord("?"), 0]
    differing, compared = cross_counts(chars_a, chars_b, ALPHABETS[name][1])
    want = _double_loop(chars_a, chars_b, ALPHABETS[name][1])
    assert differing.dtype == compared.dtype == np.uint32 and differing.shape == (m, n)
    assert np.array_equal(differing, want[0]) and np.array_equal(compared, want[1])
    if positions >= 63 and m and n:
        assert differing.max() > 0 and compared.min() < positions  # differences and not-valid symbols occur


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_cross_counts_are_the_off_diagonal_block_of_the_square(name):
    rng = np.random.default_rng(510)
    chars_a, chars_b = _draw(rng, name, 37, 150), _draw(rng, name, 90, 150)
    differing, compared = pair_counts(np.concatenate([chars_a, chars_b]), ALPHABETS[name][1])
    got = cross_counts(chars_a, chars_b, ALPHABETS[name][1])
    assert np.array_equal(got[0], differing[:37, 37:]) and np.array_equal(got[1], compared[:37, 37:])
    chunked = cross_counts(chars_a, chars_b, ALPHABETS[name][1], max_elements=1000)  # several chunks of rows
    assert np.array_equal(chunked[0], got[0]) and np.array_equal(chunked[1], got[1])
    transposed = cross_counts(chars_b, chars_a, ALPHABETS[name][1])
    assert np.array_equal(transposed[0], got[0].T) and np.array_equal(transposed[1], got[1].T)


def test_cells_apply_self_and_both_bounds():
    rng = np.random.default_rng(520)
    differing = rng.integers(0, 6, size=(5, 9), dtype=np.uint32)
    compared = rng.integers(0, 6, size=(5, 9), dtype=np.uint32)
    everything = cells_of(differing, compared, None, NOT_ELIGIBLE, 0)
    assert np.array_equal(everything[..., 0], differing) and np.array_equal(everything[..., 1], compared)
    self_columns = np.array([0, 8, 4, 9, NOT_ELIGIBLE], dtype=np.uint32)  # the first, the last, the middle, two that name no column
    for max_distance in (0, 2, 5, NOT_ELIGIBLE):
        for min_compared in (0, 3, 6, NOT_ELIGIBLE):
            cells = cells_of(differing, compared, self_columns, max_distance, min_compared)
            for i in range(5):
                for j in range(9):
                    eligible = j != self_columns[i] and differing[i, j] <= max_distance and compared[i, j] >= min_compared
                    assert cells[i, j].tolist() == ([differing[i, j], compared[i, j]] if eligible else [NOT_ELIGIBLE, NOT_ELIGIBLE])
    assert (cells_of(differing, compared, None, NOT_ELIGIBLE, 6) == NOT_ELIGIBLE).all()
    same = cells_of(differing, compared, np.array([2, 2, 2, 2, 2]), NOT_ELIGIBLE, 0)  # subjects that name the same column
    assert (same[:, 2] == NOT_ELIGIBLE).all() and (np.delete(same, 2, axis=1)[..., 0] == np.delete(differing, 2, axis=1)).all()
    assert cells_of(np.zeros((2, 0), np.uint32), np.zeros((2, 0), np.uint32), None, 0, 0).shape == (2, 0, 2)


def _lexsorted(cells, k):
    lists, counts = [], []
    for row in cells:
        columns = np.flatnonzero(row[:, 0] != NOT_ELIGIBLE)
        order = columns[np.lexsort((columns, row[columns, 0]))][:k]
        lists.append([[int(c), int(row[c, 0]), int(row[c, 1])] for c in order])
        counts.append(len(order))
    return lists, counts


@pytest.mark.parametrize("m,n,high,absent", [(1, 1, 3, 0.0), (4, 2, 1, 0.0), (6, 70, 4, 0.3), (3, 1000, 3, 0.0), (5, 300, 2**32 - 1, 0.5), (4, 50, 5, 1.0), (3, 8192, 2, 0.9)])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_nearest_columns_match_a_full_lexsort_per_row(m, n, high, absent, k):
    rng = np.random.default_rng(530 + m + n + k)
    cells = rng.integers(0, high, size=(m, n, 2), dtype=np.uint32)
    cells[rng.random((m, n)) < absent] = NOT_ELIGIBLE
    lists, counts = nearest_columns(cells, k, untouched=77)
    want_lists, want_counts = _lexsorted(cells, k)
    assert lists.dtype == counts.dtype == np.uint32 and lists.shape == (m, k, 3)
    assert counts.tolist() == want_counts
    for i in range(m):
        assert lists[i, :counts[i]].tolist() == want_lists[i] and (lists[i, counts[i]:] == 77).all()
    if high <= 5 and absent < 1.0 and n >= 8 * k:  # far more eligible cells than k over at most 5 distances
        assert any(cells[i, lists[i, counts[i] - 1, 0] + 1:, 0].tolist().count(lists[i, counts[i] - 1, 1]) for i in range(m) if counts[i] == k), "no tie at the k-th place"


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_the_two_steps_in_a_row_on_characters(name):
    rng = np.random.default_rng(540)
    chars = _draw(rng, name, 60, 120, changed=0.05)
    subjects, candidates = chars[10:30], chars[20:60]  # subjects 10 .. 19 are candidates 0 .. 9
    self_columns = np.concatenate([np.full(10, NOT_ELIGIBLE), np.arange(10)]).astype(np.uint32)
    differing, compared = _double_loop(subjects, candidates, ALPHABETS[name][1])
    d = int(np.sort(differing.ravel())[differing.size // 3])
    lists, counts = nearest_among(subjects, candidates, ALPHABETS[name][1], self_columns, 4, max_distance=d)
    fewer = 0
    for s in range(20):
        order = sorted((int(differing[s, c]), c) for c in range(40) if c != self_columns[s] and differing[s, c] <= d)[:4]
        assert counts[s] == len(order)
        assert lists[s, :len(order)].tolist() == [[c, distance, int(compared[s, c])] for distance, c in order]
        fewer += len(order) < 4
    assert 0 < fewer < 20  # the bound leaves some subjects with fewer than k


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_CROSS_ROWS == defined("SILO_GPU_MAX_CROSS_ROWS") == defined("SILO_GPU_MAX_DISTANCE_ROWS") == MAX_ROWS == 2048
    assert binding.MAX_CROSS_COLUMNS == defined("SILO_GPU_MAX_CROSS_COLUMNS") == defined("SILO_GPU_MAX_CLUSTER_ROWS") == MAX_COLUMNS == 8192
    assert binding.MAX_NEIGHBOUR_COLUMNS == defined("SILO_GPU_MAX_NEIGHBOUR_COLUMNS") == MAX_NEIGHBOURS == 64
    assert binding.NEIGHBOUR_THREADS == defined("SILO_GPU_NEIGHBOUR_THREADS") == 1024
    assert binding.NEIGHBOUR_KEY_COLUMN_BITS == defined("SILO_GPU_NEIGHBOUR_KEY_COLUMN_BITS") == COLUMN_BITS
    assert 1 << COLUMN_BITS == binding.MAX_CROSS_COLUMNS and binding.MAX_CROSS_COLUMNS % binding.NEIGHBOUR_THREADS == 0
    assert binding.NOT_ELIGIBLE == NOT_ELIGIBLE == 2**32 - 1
    for name in ("silo_gpu_distance_cross", "silo_gpu_nearest_columns"):
        assert name in binding.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", header)
