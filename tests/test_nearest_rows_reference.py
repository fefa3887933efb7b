"""tests/nearest_rows_reference.py against plain loops and against pair_distances, and the constants silo_amd/binding.py restates
against include/silo_gpu.h.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import nearest_rows_reference as ref
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID, pair_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}


def _chars(rng, n, positions, all_chars):
    pool = np.frombuffer((all_chars + "a?.U\0").encode("latin-1"), dtype=np.uint8)
    return pool[rng.integers(0, len(pool), size=(n, positions))]


def _loop_distances(chars, query, valid_chars):
    out = np.zeros((len(chars), 2), dtype=np.uint32)
    for r, row in enumerate(chars):
        for a, b in zip(row.tobytes().decode("latin-1"), query.tobytes().decode("latin-1")):
            if a in valid_chars and b in valid_chars:
                out[r, 1] += 1
                out[r, 0] += a != b
    return out


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_query_distances_match_the_character_loop(alphabet):
    all_chars, valid = ALPHABETS[alphabet]
    rng = np.random.default_rng(7 + len(valid))
    chars = _chars(rng, 37, 53, all_chars)
    for query in (chars[5], _chars(rng, 1, 53, all_chars)[0], np.full(53, ord("N"), np.uint8), np.zeros(53, np.uint8)):
        assert np.array_equal(ref.query_distances(chars, query, valid), _loop_distances(chars, query, valid))
    assert not ref.query_distances(chars, np.full(53, ord("X" if alphabet == "aa" else "N"), np.uint8), valid).any()
    assert ref.query_distances(chars[:0], chars[0], valid).shape == (0, 2)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_query_distances_are_rows_of_pair_distances(alphabet):
    all_chars, valid = ALPHABETS[alphabet]
    rng = np.random.default_rng(11 + len(valid))
    chars = _chars(rng, 29, 131, all_chars)
    square = pair_distances(chars, valid)
    for i in range(len(chars)):
        assert np.array_equal(ref.query_distances(chars, chars[i], valid), square[i])


def _sorted_everything(table, mask, k, max_distance, exclude):
    keys = []
    for row in range(len(table)):
        if mask is not None and not mask[row]:
            continue
        if exclude is not None and row == exclude:
            continue
        if max_distance is not None and table[row][0] > max_distance:
            continue
        keys.append((int(table[row][0]), row))
    return [row for _, row in sorted(keys)[:k]]


def test_nearest_matches_sorting_everything():
    rng = np.random.default_rng(3)
    tables = {
        "random": rng.integers(0, 1 << 20, size=(500, 2)).astype(np.uint32),
        "ties": np.column_stack([rng.integers(0, 3, size=700), rng.integers(0, 9, size=700)]).astype(np.uint32),  # massive ties
        "one": np.array([[4, 9]], dtype=np.uint32),
    }
    for name, table in tables.items():
        n = len(table)
        for mask in (None, rng.random(n) < 0.5, np.zeros(n, bool)):
            for k in (1, 10, n, n + 5):
                for max_distance in (None, 0, 1, 1 << 19):
                    for exclude in (None, 0, n - 1, ref.NO_ROW):
                        got = ref.nearest(table, mask, k, max_distance, exclude)
                        want = _sorted_everything(table, mask, k, max_distance, None if exclude == ref.NO_ROW else exclude)
                        assert got.tolist() == want, (name, k, max_distance, exclude)
    listed = ref.nearest_list(tables["ties"], ref.nearest(tables["ties"], None, 10))
    assert listed.dtype == np.uint32 and listed.shape == (10, 3)
    assert np.array_equal(listed[:, 1:], tables["ties"][listed[:, 0]])


def _header_number(name):
    with open(os.path.join(ROOT, "include", "silo_gpu.h"), encoding="utf-8") as header:
        found = re.search(r"#define\s+" + name + r"\s+(\d+)", header.read())
    assert found is not None, name
    return int(found.group(1))


def test_binding_restates_the_header():
    from silo_amd import binding

    assert binding.MAX_NEAREST_ROWS == _header_number("SILO_GPU_MAX_NEAREST_ROWS") == 1024
    assert binding.NEAREST_ROWS_SCRATCH_BYTES == _header_number("SILO_GPU_NEAREST_ROWS_SCRATCH_BYTES")
    assert binding.QUERY_DISTANCE_COUNTER_PLANES == _header_number("SILO_GPU_QUERY_DISTANCE_COUNTER_PLANES")
    with open(os.path.join(ROOT, "include", "silo_gpu.h"), encoding="utf-8") as header:
        text = header.read().replace("\\\n", " ")
    macro = re.search(r"#define\s+SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES\(positions\)\s+(.*)", text).group(1)
    expression = re.sub(r"\(size_t\)", "", macro).replace("u", "").replace("/", "//")
    for positions in (0, 1, 24, 255, 256, 257, 1273, 29_903, 66_000):
        assert binding.query_distance_scratch_bytes(positions) == eval(expression, {"positions": positions})  # noqa: S307
        # what the entry lays out: the query's symbols, then two prefix arrays of positions + 1 words, each on a 256-byte line
        assert binding.query_distance_scratch_bytes(positions) >= -(-positions // 256) * 256 + 2 * (-(-(positions + 1) * 4 // 256) * 256)
