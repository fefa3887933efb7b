"""tests/pair_distances_reference.py (the numpy reference of K10) against a plain Python double loop, and the constants of K10 that
silo_amd/binding.py restates against include/silo_gpu.h; runs without a GPU."""
import os
import re

import numpy as np
import pytest

from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID, code_bits, pack_planes, pair_distances

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}


def _loop(rows, valid_chars):
    """The definition, character by character."""
    n = len(rows)
    out = np.zeros((n, n, 2), dtype=np.uint32)
    for i in range(n):
        for j in range(n):
            for a, b in zip(rows[i], rows[j]):
                if a in valid_chars and b in valid_chars:
                    out[i, j, 1] += 1
                    out[i, j, 0] += a != b
    return out


def _matrix(rows):
    return np.array([list(row.encode("latin-1")) for row in rows], dtype=np.uint8).reshape(len(rows), -1)


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_pair_distances_match_a_double_loop(name):
    """9 rows of 75 characters drawn from the whole alphabet, most positions agreeing; in one chunk and in chunks of two rows."""
    all_chars, valid_chars = ALPHABETS[name]
    rng = np.random.default_rng(101)
    base = rng.choice(list(valid_chars), size=75)
    rows = []
    for _ in range(9):
        row = base.copy()
        changed = rng.random(75) < 0.3
        row[changed] = rng.choice(list(all_chars), size=int(changed.sum()))
        rows.append("".join(row))
    want = _loop(rows, valid_chars)
    for max_elements in (1 << 25, 2 * 9 * 75):
        got = pair_distances(_matrix(rows), valid_chars, max_elements)
        assert got.dtype == np.uint32 and got.shape == (9, 9, 2)
        assert np.array_equal(got, want)
    assert np.array_equal(want, want.transpose(1, 0, 2)) and not want[:, :, 0].diagonal().any()
    assert want[:, :, 0].max() > 3 and (want[:, :, 1] < 75).any() and (want[:, :, 0] <= want[:, :, 1]).all()
    assert pair_distances(np.zeros((0, 75), np.uint8), valid_chars).shape == (0, 0, 2)
    assert not pair_distances(np.zeros((3, 0), np.uint8), valid_chars).any()


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_rows_of_the_missing_symbol_and_bytes_outside_the_alphabet(name):
    all_chars, valid_chars = ALPHABETS[name]
    missing = all_chars[-1]  # N / X
    assert missing in "NX" and missing not in valid_chars
    ordinary = (valid_chars * 4)[:20]
    shifted = ordinary[1:] + ordinary[:1]  # valid everywhere, differs everywhere
    strange = "a?\0" + ordinary[3:17] + "\xff~ "  # bytes that are no symbol of the alphabet
    rows = [missing * 20, ordinary, shifted, strange, ordinary]
    got = pair_distances(_matrix(rows), valid_chars)
    assert np.array_equal(got, _loop(rows, valid_chars))
    assert not got[0].any() and not got[:, 0].any()                     # the missing row against anything, itself included
    assert got[1, 2].tolist() == [20, 20] and got[1, 4].tolist() == [0, 20]
    assert got[3, 3].tolist() == [0, 14] and got[1, 3].tolist() == [0, 14] and got[2, 3].tolist() == [14, 14]


@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_pack_planes_hold_valid_bits_and_codes(name):
    all_chars, valid_chars = ALPHABETS[name]
    rng = np.random.default_rng(102)
    positions = 131
    chars = _matrix(["".join(rng.choice(list(all_chars + "a?"), size=positions)) for _ in range(3)])
    planes = pack_planes(chars, valid_chars)
    assert planes.dtype == np.uint64 and planes.shape == (3, 1 + code_bits(valid_chars), 3)
    for r in range(3):
        for p in range(positions + 61):
            bits = [int(planes[r, k, p // 64] >> np.uint64(p % 64)) & 1 for k in range(planes.shape[1])]
            char = chr(chars[r, p]) if p < positions else None
            if char is not None and char in valid_chars:
                assert bits[0] == 1 and sum(bit << k for k, bit in enumerate(bits[1:])) == valid_chars.index(char)
            else:
                assert not any(bits)


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_DISTANCE_ROWS == defined("SILO_GPU_MAX_DISTANCE_ROWS") == 2048
    assert binding.DISTANCE_TILE == defined("SILO_GPU_DISTANCE_TILE")
    assert binding.DISTANCE_CHUNK_WORDS == defined("SILO_GPU_DISTANCE_CHUNK_WORDS")
    assert (binding.distance_planes("nuc"), binding.distance_planes("aa")) == (1 + code_bits(NUC_VALID), 1 + code_bits(AA_VALID)) == (4, 6)
    assert [binding.distance_words(p) for p in (1, 64, 65, 29_903)] == [1, 1, 2, 468]
