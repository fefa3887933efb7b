"""tests/haplotypes_reference.py (the numpy reference of K16 and of the Haplotypes action) against a plain Python double loop with a
dict counter, against rows worked out by hand, and the constants of K16 that silo_amd/binding.py restates against
include/silo_gpu.h; runs without a GPU."""
import os
import re

import numpy as np
import pytest

from tests.haplotypes_reference import (
    ALL_COMPLETE, MAX_POSITIONS, POSITIONS_PER_COLUMN, SYMBOL_NONE, complete_rows, haplotype_ids, haplotype_rows, mask_of, padded_rows,
    position_symbols,
)

NUC = "-ACGTRYSWKMBDHVN"
AA = "-ACDEFGHIKLMNPQRSTVWYBZ*X"
NUC_VALID = [0, 1, 2, 3, 4]
AA_VALID = list(range(21)) + [23]


def ids_of(text, chars):
    return np.array([[chars.index(c) for c in row] for row in text], dtype=np.uint8)


def by_key(rows):
    return {(row["groups"], row["haplotype"]): (row["count"], row["proportion"]) for row in rows}


@pytest.mark.parametrize("chars,valid", [(NUC, NUC_VALID), (AA, AA_VALID)], ids=["nuc", "aa"])
@pytest.mark.parametrize("exclude", [False, True])
def test_rows_match_a_double_loop_with_a_dict(chars, valid, exclude):
    rng = np.random.default_rng(len(chars) + exclude)
    n, width = 300, 9
    sym = rng.choice(len(chars), size=(n, width), p=np.r_[[0.5, 0.3], np.full(len(chars) - 2, 0.2 / (len(chars) - 2))]).astype(np.uint8)
    mask = rng.random(n) < 0.7
    groups = [(int(g), "x" if g % 2 else None) for g in rng.integers(0, 3, size=n)]
    positions = [7, 0, 3]
    counter = {}
    for row in range(n):
        if not mask[row]:
            continue
        letters = ""
        complete = True
        for position in positions:
            letters += chars[sym[row, position]]
            complete = complete and sym[row, position] in valid
        if exclude and not complete:
            continue
        counter[(groups[row], letters)] = counter.get((groups[row], letters), 0) + 1
    total = sum(counter.values())
    rows = haplotype_rows(sym, positions, chars, mask=mask, valid_symbols=valid if exclude else None, groups=groups)
    assert by_key(rows) == {key: (count, count / total) for key, count in counter.items()}
    assert len(counter) > 6 and abs(sum(row["proportion"] for row in rows) - 1.0) < 1e-12
    if exclude:  # what excludeIncomplete leaves out: exactly the rows with another symbol at a listed position
        everything = haplotype_rows(sym, positions, chars, mask=mask, groups=groups)
        kept = {key: value[0] for key, value in by_key(everything).items() if all(chars.index(c) in valid for c in key[1])}
        assert kept == {key: value[0] for key, value in by_key(rows).items()} and len(everything) > len(rows)


def test_hand_made_rows():
    text = ["ACGTAC", "ACGTAC", "NNNNNN", "RCGTAC", "ACGTAY", "-CGTAC"]
    sym = ids_of(text, NUC)
    # k = 1
    assert by_key(haplotype_rows(sym, [0], NUC)) == {((), "A"): (3, 0.5), ((), "N"): (1, 1 / 6), ((), "R"): (1, 1 / 6), ((), "-"): (1, 1 / 6)}
    # the duplicated row counts twice; the row of only the missing symbol is a haplotype of its own
    rows = by_key(haplotype_rows(sym, [0, 1, 5], NUC))
    assert rows == {((), "ACC"): (2, 2 / 6), ((), "NNN"): (1, 1 / 6), ((), "RCC"): (1, 1 / 6), ((), "ACY"): (1, 1 / 6), ((), "-CC"): (1, 1 / 6)}
    # an ambiguity code at the first listed position, one at the last, the missing row: left out by excludeIncomplete
    assert by_key(haplotype_rows(sym, [0, 1, 5], NUC, valid_symbols=NUC_VALID)) == {((), "ACC"): (2, 2 / 3), ((), "-CC"): (1, 1 / 3)}
    # request order is kept, a filter that selects nothing gives no row
    assert by_key(haplotype_rows(sym, [5, 0], NUC, mask=[True, False, False, False, True, False])) == {((), "CA"): (1, 0.5), ((), "YA"): (1, 0.5)}
    assert haplotype_rows(sym, [0], NUC, mask=np.zeros(6, dtype=bool)) == []


def test_symbol_columns_and_padding():
    sym = ids_of(["ACGT", "NNCA", "-RTT"], NUC)
    columns = position_symbols(sym, [3, 0, 3])
    assert columns.shape == (3, 2048) == (3, padded_rows(3)) and padded_rows(2048) == 2048 and padded_rows(2049) == 4096
    assert columns[:, :3].tolist() == [[4, 1, 4], [1, 15, 0], [4, 1, 4]] and (columns[:, 3:] == SYMBOL_NONE).all()


@pytest.mark.parametrize("k", [6, 7])
def test_the_column_boundary(k):
    """k = 6 fills one column to its last digit, k = 7 opens the second with a single digit."""
    sym = ids_of(["TTTTTTT", "ACGTACG", "NNNNNNN"], NUC)
    symbols = position_symbols(sym, list(range(k)), rows=64)
    ids = haplotype_ids(symbols, 3, 16)
    assert ids.shape == ((k + 5) // 6, 64)
    assert ids[0, :3].tolist() == [0x444444, 0x123412, 0xFFFFFF] and not ids[:, 3:].any()
    if k == 7:
        assert ids[1, :3].tolist() == [4, 3, 15]


def test_twelve_amino_acid_positions_are_the_largest_tuple_space():
    assert 25**12 < 2**64 - 1 and 25**POSITIONS_PER_COLUMN < 2**28 and 16**POSITIONS_PER_COLUMN == 2**24
    sym = ids_of(["XXXXXXXXXXXX", "-ACDEFGHIKLM", "************"], AA)
    ids = haplotype_ids(position_symbols(sym, list(range(12)), rows=64), 3, 25)
    assert ids.shape == (2, 64)
    assert ids[:, 0].tolist() == [25**6 - 1, 25**6 - 1]
    assert ids[0, 1] == sum(d * 25 ** (5 - i) for i, d in enumerate(range(6))) and ids[1, 1] == sum(d * 25 ** (5 - i) for i, d in enumerate(range(6, 12)))
    assert int(ids[0, 0]) * 25**6 + int(ids[1, 0]) == 25**12 - 1
    rows = haplotype_rows(sym, list(range(12)), AA, valid_symbols=AA_VALID)
    assert [row["haplotype"] for row in rows] == ["************", "-ACDEFGHIKLM"] or [row["haplotype"] for row in rows] == ["-ACDEFGHIKLM", "************"]


def test_ids_of_rows_without_a_symbol_and_the_row_bitset():
    symbols = np.array([[1, 2, SYMBOL_NONE, 15, 1, 7], [4, 4, 4, 4, 16, 1]], dtype=np.uint8)
    symbols = np.concatenate([symbols, np.full((2, 58), 1, dtype=np.uint8)], axis=1)
    ids = haplotype_ids(symbols, 6, 16)
    # row 2 holds SYMBOL_NONE, row 4 a byte that is no nucleotide id: 0 in all columns; the rows at or past sequence_count too
    assert ids[0, :8].tolist() == [0x14, 0x24, 0, 0xF4, 0, 0x71, 0, 0]
    every = np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    assert complete_rows(symbols, 6, ALL_COMPLETE, every).tolist() == [0b111111]  # the filter, masked to the real rows
    assert complete_rows(symbols, 6, ALL_COMPLETE, None).tolist() == [0b111111]
    assert complete_rows(symbols, 6, mask_of(NUC_VALID), every).tolist() == [0b000011]  # N, R, SYMBOL_NONE and the byte 16 are not valid
    assert complete_rows(symbols, 6, mask_of(NUC_VALID), np.array([0b10], dtype=np.uint64)).tolist() == [0b10]
    assert mask_of(NUC_VALID) == 0b11111 and mask_of(AA_VALID) == (1 << 21) - 1 + (1 << 23)


def test_the_binding_restates_the_constants_of_the_header():
    from silo_amd import binding

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "silo_gpu.h")).read()

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(0x[0-9A-Fa-f]+|\d+)", header).group(1), 0)

    assert binding.MAX_HAPLOTYPE_POSITIONS == defined("SILO_GPU_MAX_HAPLOTYPE_POSITIONS") == MAX_POSITIONS == 12
    assert binding.HAPLOTYPE_POSITIONS_PER_COLUMN == defined("SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN") == POSITIONS_PER_COLUMN == 6
    assert binding.SYMBOL_NONE == defined("SILO_GPU_SYMBOL_NONE") == SYMBOL_NONE and binding.ALL_SYMBOLS_COMPLETE == ALL_COMPLETE
    # the id columns of the largest request, behind the most groupByFields the action takes, are within the group-by's columns
    assert 6 + -(-MAX_POSITIONS // POSITIONS_PER_COLUMN) <= defined("SILO_GPU_MAX_GROUP_COLUMNS")
    for name in ("silo_gpu_position_symbols", "silo_gpu_haplotype_ids"):
        assert name in binding.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", header)
