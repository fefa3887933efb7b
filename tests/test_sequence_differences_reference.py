"""tests/sequence_differences_reference.py (the numpy reference of K18 and of the rows of MutationsPerSequence) against a plain loop
over rows and positions that applies the rule on its own, against rows worked out by hand, the constants of K18 that
silo_amd/binding.py restates against include/silo_gpu.h, and the numbers the reference gives on the oracle's FastaAligned strings of
the example data set; runs without a GPU."""
import os
import re

import numpy as np
import pytest

from oracle import silo_oracle as so
from tests import dataset
from tests.sequence_differences_reference import (AMBIGUOUS, CHUNK, COUNT_FIELDS, DELETION, FIRST_WORDS_PER_ROW, HAND_MADE, LIST_FIELDS, MAX_POSITIONS,
                                                  MAX_ROWS, MISSING, MISSING_SYMBOL, QUAD, SAME, STATS, SUBSTITUTION, VALID, classify,
                                                  difference_records, hand_made_matrix, response_rows, row_fields, skewed_chars)
from tests.test_oracle_golden import build_oracle_db

# what a numpy run of the rule gave on the oracle's strings (100 rows): words, substitution / deleted / missing / ambiguous cells,
# rows that begin inside a run, rows that end inside one, rows without a word
EXAMPLE = {"main": ("nuc", 4786, (3033, 6691, 60723, 35), 99, 95, 0), "S": ("aa", 1777, (1371, 1667, 3031, 0), 3, 2, 1)}


def _loop_class(c, r, alphabet):
    if c == ord(MISSING_SYMBOL[alphabet]):
        return MISSING
    if chr(c) not in VALID[alphabet]:
        return AMBIGUOUS
    if c == r:
        return SAME
    return DELETION if c == ord("-") else SUBSTITUTION


def _loop(chars, reference, alphabet):
    """(classes, offsets, stats, words) by the rule as the issue words it, a cell at a time."""
    classes, offsets, stats, words = [], [0], [], []
    for row in chars:
        of_row, counts, previous = [], [0, 0, 0, 0], None
        for p, (c, r) in enumerate(zip(row, reference)):
            mine = _loop_class(c, r, alphabet)
            of_row.append(mine)
            if mine in (SUBSTITUTION, AMBIGUOUS):
                words.append((p << 9) | c)
            elif mine in (DELETION, MISSING):
                if p == 0 or previous != mine:
                    words.append((p << 9) | c)
            elif p > 0 and previous in (DELETION, MISSING):
                words.append((p << 9) | 0x100)
            if mine != SAME:
                counts[(SUBSTITUTION, DELETION, MISSING, AMBIGUOUS).index(mine)] += 1
            previous = mine
        classes.append(of_row)
        offsets.append(len(words))
        stats.append(counts)
    return classes, offsets, stats, words


def _loop_fields(row, reference, alphabet):
    """The response's fields of one row by a walk over its cells."""
    lists = {field: [] for field in LIST_FIELDS}
    counts = dict.fromkeys(COUNT_FIELDS, 0)
    run = None  # (field, first)
    for p in range(len(row) + 1):
        mine = _loop_class(row[p], reference[p], alphabet) if p < len(row) else None
        field = {DELETION: "deletions", MISSING: "missing"}.get(mine)
        if run is not None and run[0] != field:
            lists[run[0]].append(str(run[1] + 1) if p - run[1] == 1 else f"{run[1] + 1}-{p}")
            run = None
        if field is not None and run is None:
            run = (field, p)
        if mine in (SUBSTITUTION, AMBIGUOUS):
            lists["substitutions" if mine == SUBSTITUTION else "ambiguous"].append(chr(reference[p]) + str(p + 1) + chr(row[p]))
        if mine not in (None, SAME):
            counts[COUNT_FIELDS[(SUBSTITUTION, DELETION, MISSING, AMBIGUOUS).index(mine)]] += 1
    return dict({field: ",".join(items) for field, items in lists.items()}, **counts)


def _same(chars, reference, alphabet):
    classes, offsets, stats, words = _loop(chars.tolist(), reference.tolist(), alphabet)
    assert classify(chars, reference, alphabet).tolist() == classes
    got_offsets, got_stats, got_words = difference_records(chars, reference, alphabet)
    assert got_offsets.dtype == got_stats.dtype == got_words.dtype == np.uint32 and got_stats.shape == (len(chars), STATS)
    assert got_offsets.tolist() == offsets and got_stats.tolist() == stats and got_words.tolist() == words
    for row in chars:
        assert row_fields(row, reference, alphabet) == _loop_fields(row.tolist(), reference.tolist(), alphabet)
    return len(words)


@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
@pytest.mark.parametrize("rows,positions", [(1, 1), (3, 17), (7, 400), (20, 90)])
def test_random_matrices_match_a_plain_loop(alphabet, rows, positions):
    rng = np.random.default_rng(1800 + rows + positions)
    chars, reference = skewed_chars(rng, alphabet, rows, positions)
    words = _same(chars, reference, alphabet)
    classes = classify(chars, reference, alphabet)
    if rows * positions >= 1000:  # not vacuous: every class occurs, and a row ends in a run where the next begins with one
        assert set(np.unique(classes).tolist()) == {SAME, SUBSTITUTION, DELETION, MISSING, AMBIGUOUS} and 0 < words < rows * positions // 4
        assert any(classes[r, -1] == classes[r + 1, 0] and classes[r, -1] in (DELETION, MISSING) for r in range(rows - 1)) or rows < 20


@pytest.mark.parametrize("case", range(len(HAND_MADE)))
def test_hand_made_rows(case):
    what, alphabet = HAND_MADE[case][:2]
    chars, reference, words = hand_made_matrix(HAND_MADE[case])
    assert difference_records(chars, reference, alphabet)[2].tolist() == words.tolist(), what
    _same(chars, reference, alphabet)


def test_the_fields_of_a_row():
    reference = "ACGTACGTACGTN"
    row = np.frombuffer(b"--GAYC---CGNN", dtype=np.uint8)
    assert row_fields(row, reference, "nuc") == {
        "substitutions": "T4A", "deletions": "1-2,7-9", "missing": "12-13", "ambiguous": "A5Y", "substitutionCount": 1, "deletedPositions": 5,
        "missingPositions": 2, "ambiguousPositions": 1}
    same = np.frombuffer(reference[:12].encode(), dtype=np.uint8)
    assert row_fields(same, reference[:12], "nuc") == dict({field: "" for field in LIST_FIELDS}, **dict.fromkeys(COUNT_FIELDS, 0))
    assert row_fields(np.frombuffer(b"ACGN", dtype=np.uint8), "ACGT", "nuc")["missing"] == "4"
    rows = response_rows(["k1", "k2"], np.stack([same, same]), reference[:12], "nuc", "main", "key")
    assert [row["key"] for row in rows] == ["k1", "k2"] and set(rows[0]) == {"key", "sequenceName", *LIST_FIELDS, *COUNT_FIELDS} and rows[1]["sequenceName"] == "main"


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        text = re.search(r"#define\s+" + name + r"\s+(\(1u << \d+\)|\d+)", header).group(1)
        shift = re.fullmatch(r"\(1u << (\d+)\)", text)
        return 1 << int(shift.group(1)) if shift else int(text)

    assert binding.MAX_DIFFERENCE_ROWS == defined("SILO_GPU_MAX_DIFFERENCE_ROWS") == MAX_ROWS == 10_000
    assert binding.MAX_DIFFERENCE_POSITIONS == defined("SILO_GPU_MAX_DIFFERENCE_POSITIONS") == MAX_POSITIONS == 1 << 23
    assert binding.DIFFERENCE_STATS == defined("SILO_GPU_DIFFERENCE_STATS") == STATS == 4
    assert binding.DIFFERENCE_CHUNK == defined("SILO_GPU_DIFFERENCE_CHUNK") == CHUNK == 256 * QUAD
    assert FIRST_WORDS_PER_ROW == 32
    for positions in (0, 1, CHUNK - 15, CHUNK - 14, CHUNK, 29_903, MAX_POSITIONS):  # a row starts up to 15 bytes past a 16-byte boundary
        chunks = binding.difference_chunks(positions)
        assert (chunks - 1) * CHUNK < positions + 15 <= chunks * CHUNK or positions == 0 and chunks == 1
        assert binding.differences_scratch_bytes(7, positions) == 7 * chunks * (1 + STATS) * 4
    assert "silo_gpu_sequence_differences" in binding.EXPORTED_SYMBOLS and re.search(r"\bint silo_gpu_sequence_differences\(", header)
    assert re.search(r"#define\s+SILO_GPU_DIFFERENCES_SCRATCH_BYTES\(n_rows, positions\)", header)


@pytest.fixture(scope="module")
def oracle_strings():
    data = dataset.load_example_dataset()
    oracle_db = build_oracle_db(data, None)
    out = {}
    for store in EXAMPLE:
        selected = so.execute_query(oracle_db, {"action": {"type": "FastaAligned", "sequenceName": store}, "filterExpression": {"type": "True"}})
        out[store] = np.array([list(row[store].encode()) for row in selected], dtype=np.uint8)
    return data, out


@pytest.mark.parametrize("store", sorted(EXAMPLE))
def test_the_example_data_set_gives_the_numbers_the_tests_rely_on(oracle_strings, store):
    data, strings = oracle_strings
    alphabet, n_words, cells, begin_inside, end_inside, without_word = EXAMPLE[store]
    chars = strings[store]
    reference = (data["nuc_references"] if alphabet == "nuc" else data["aa_references"])[store]
    assert chars.shape == (100, len(reference))
    offsets, stats, words = difference_records(chars, reference, alphabet)
    assert len(words) == offsets[-1] == n_words and tuple(stats.sum(axis=0).tolist()) == cells
    classes = classify(chars, reference, alphabet)
    assert int(np.isin(classes[:, 0], (DELETION, MISSING)).sum()) == begin_inside
    assert int(np.isin(classes[:, -1], (DELETION, MISSING)).sum()) == end_inside
    assert int((np.diff(offsets.astype(np.int64)) == 0).sum()) == without_word
    per_row = np.diff(offsets.astype(np.int64))
    if store == "main":
        assert (int(per_row.min()), int(np.median(per_row)), int(per_row.max())) == (11, 47, 185)
        ambiguous = chars[classes == AMBIGUOUS]
        assert sorted(set(bytes(ambiguous).decode())) == list("KMRWY") and int((classes == AMBIGUOUS).any(axis=1).sum()) == 7
        assert n_words > FIRST_WORDS_PER_ROW * 100  # the action's second call runs
    else:
        assert (int(per_row.min()), int(np.median(per_row)), int(per_row.max())) == (0, 12, 59)
        assert n_words < FIRST_WORDS_PER_ROW * 100  # ... and does not here
    for r in (0, 37, 99):
        fields = row_fields(chars[r], reference, alphabet)
        assert [fields[field] for field in COUNT_FIELDS] == stats[r].tolist()
        assert sum(len(fields[field].split(",")) for field in ("substitutions", "ambiguous") if fields[field]) == stats[r, 0] + stats[r, 3]
