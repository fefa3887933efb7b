"""tests/consensus_reference.py (the numpy reference of K15) against a plain character double loop that counts per column, sorts
and applies the prefix-with-ties rule on its own, against rows worked out by hand, and the constants of K15 that
silo_amd/binding.py restates against include/silo_gpu.h; runs without a GPU."""
import math
import os
import re

import numpy as np
import pytest

from tests.consensus_reference import (AMBIGUOUS, CALL_CHARS, DELETED, DIFFERENCES, HAND_MADE, IUPAC, LOW_COVERAGE, MAX_TABLES, MISSING, THREADS,
                                       VALID, call_consensus, consensus_row, count_table, reference_index_of)
from tests.pair_distances_reference import AA_CHARS, NUC_CHARS

ALL_CHARS = {"nuc": NUC_CHARS, "aa": AA_CHARS}
THRESHOLDS = (0.5, 0.75, 0.9, 1.0, 1e-9)


def _loop_call(column, alphabet, threshold, min_depth):
    """(character, kind, the called symbols) of one column of characters, by the rule as the issue words it."""
    tally = {}
    for char in column:
        if char in VALID[alphabet]:
            tally[char] = tally.get(char, 0) + 1
    depth = sum(tally.values())
    if depth < min_depth:
        return MISSING[alphabet], "low", ""
    need = math.ceil(depth * threshold)
    ordered = sorted(tally.items(), key=lambda item: -item[1])
    prefix, total = [], 0
    for char, count in ordered:
        if total >= need and count != prefix[-1][1]:
            break
        prefix.append((char, count))
        total += count
    called = "".join(sorted(char for char, _ in prefix))
    if len(called) == 1:
        return called, "deleted" if called == "-" else "single", called
    if alphabet == "aa":
        return "X", "ambiguous", called
    return ("N" if "-" in called else IUPAC["".join(c for c in "ACGT" if c in called)]), "ambiguous", called


def _draw(rng, alphabet, n, positions):
    """Characters uint8 [n][positions]: columns with one heavy symbol, with two or three near-equal ones, and noisy ones."""
    every = np.frombuffer(ALL_CHARS[alphabet].encode(), dtype=np.uint8)
    valid = np.frombuffer(VALID[alphabet].encode(), dtype=np.uint8)
    chars = np.empty((n, positions), dtype=np.uint8)
    for p in range(positions):
        few = rng.choice(valid, size=rng.integers(1, 4), replace=False)
        chars[:, p] = rng.choice(few, size=n)
        noisy = rng.random(n) < rng.choice([0.0, 0.1, 0.6])
        chars[noisy, p] = rng.choice(every, size=int(noisy.sum()))
    return chars


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("n,positions", [(1, 5), (2, 40), (6, 80), (12, 120), (40, 60)])
def test_calls_match_a_character_double_loop(alphabet, n, positions):
    rng = np.random.default_rng(700 + n + positions)
    chars = _draw(rng, alphabet, n, positions)
    reference = "".join(rng.choice(list(ALL_CHARS[alphabet]), size=positions))
    kinds_seen = set()
    for threshold in THRESHOLDS:
        for min_depth in (1, max(1, n // 2), n, n + 1):
            got = consensus_row(chars, reference, alphabet, threshold, min_depth)
            want = [_loop_call(bytes(chars[:, p]).decode("latin-1"), alphabet, threshold, min_depth) for p in range(positions)]
            assert got["consensus"] == "".join(call for call, _, _ in want)
            kinds = [kind for _, kind, _ in want]
            assert got["ambiguousPositions"] == kinds.count("ambiguous") and got["lowCoveragePositions"] == kinds.count("low")
            assert got["deletedPositions"] == kinds.count("deleted") and got["count"] == n
            assert got["differences"] == sum(kind in ("single", "deleted") and call != reference[p] for p, (call, kind, _) in enumerate(want))
            assert set(got["consensus"]) <= set(CALL_CHARS[alphabet])
            kinds_seen |= set(kinds)
    if n >= 6:
        assert kinds_seen >= {"single", "ambiguous", "low"}


@pytest.mark.parametrize("row", range(len(HAND_MADE)))
def test_hand_made_rows(row):
    alphabet, counts, threshold, min_depth, call, kind = HAND_MADE[row]
    for reference_index in (0, 1, len(VALID[alphabet]) - 1, 0xFF):
        chars, summary = call_consensus(np.array([counts], dtype=np.uint32), np.array([reference_index], dtype=np.uint8), alphabet, threshold, min_depth)
        assert chr(chars[0]) == call
        assert summary[AMBIGUOUS] == (kind == "ambiguous") and summary[LOW_COVERAGE] == (kind == "low") and summary[DELETED] == (kind == "deleted")
        differs = kind in ("single", "deleted") and VALID[alphabet].index(call) != reference_index
        assert summary[DIFFERENCES] == differs


def test_the_hand_made_rows_cover_what_the_rule_distinguishes():
    nuc_calls = {call for alphabet, _, _, _, call, kind in HAND_MADE if alphabet == "nuc" and kind != "low"}
    assert nuc_calls >= set(IUPAC.values()) | {"-"}  # each of the 11 codes, the four bases, a deletion
    assert {threshold for _, _, threshold, _, _, _ in HAND_MADE} >= set(THRESHOLDS)
    assert {kind for _, _, _, _, _, kind in HAND_MADE} == {"single", "ambiguous", "low", "deleted"}
    assert any(max(counts) == 2**32 - 1 for _, counts, _, _, _, _ in HAND_MADE)


def test_tables_in_front_and_shapes():
    rng = np.random.default_rng(710)
    counts = rng.integers(0, 4, size=(3, 17, 5), dtype=np.uint32)
    reference_index = rng.integers(0, 5, size=17).astype(np.uint8)
    chars, summary = call_consensus(counts, reference_index, "nuc", 0.75, 2)
    assert chars.shape == (3, 17) and chars.dtype == np.uint8 and summary.shape == (3, 4) and summary.dtype == np.uint32
    for t in range(3):
        one_chars, one_summary = call_consensus(counts[t], reference_index, "nuc", 0.75, 2)
        assert np.array_equal(chars[t], one_chars) and np.array_equal(summary[t], one_summary)
    empty_chars, empty_summary = call_consensus(np.zeros((2, 0, 22), np.uint32), np.zeros(0, np.uint8), "aa", 0.5, 1)
    assert empty_chars.shape == (2, 0) and not empty_summary.any()
    assert (summary[:, AMBIGUOUS] + summary[:, LOW_COVERAGE] + summary[:, DELETED] <= 17).all()


def test_count_table_and_reference_index():
    chars = np.frombuffer(b"AC-N" b"ACGa" b"TC-\x00", dtype=np.uint8).reshape(3, 4)
    assert count_table(chars, "nuc").tolist() == [[0, 2, 0, 0, 1], [0, 0, 3, 0, 0], [2, 0, 0, 1, 0], [0, 0, 0, 0, 0]]
    assert reference_index_of("-ACGTN", "nuc").tolist() == [0, 1, 2, 3, 4, 0xFF]
    assert reference_index_of("-Y*XB", "aa").tolist() == [0, 20, 21, 0xFF, 0xFF]


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))

    assert binding.MAX_CONSENSUS_TABLES == defined("SILO_GPU_MAX_CONSENSUS_TABLES") == MAX_TABLES == 64
    assert binding.CONSENSUS_THREADS == defined("SILO_GPU_CONSENSUS_THREADS") == THREADS == 256
    assert binding.CONSENSUS_SUMMARY_WORDS == 4 == len({AMBIGUOUS, LOW_COVERAGE, DELETED, DIFFERENCES})
    assert "silo_gpu_consensus_call" in binding.EXPORTED_SYMBOLS and re.search(r"\bint silo_gpu_consensus_call\(", header)
