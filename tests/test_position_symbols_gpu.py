"""The symbol columns of K16 (csrc/silo_gpu_haplotypes.hip) through their entries, silo_gpu_position_symbols and
silo_gpu_haplotype_ids, against the plain numpy reference of tests/haplotypes_reference.py (pinned without a GPU by
tests/test_haplotypes_reference.py).

silo_gpu_position_symbols reads whole cells off the adaptive layout, so it gets the stores of tests/test_grouped_kernels_gpu.py in
each of the five layouts (derived symbols, one-hot rows, code planes, identity planes, a resident plane of the missing symbol), both
alphabets, and small stores around the sizes where a word, a 256-byte line and the row padding end.  silo_gpu_haplotype_ids takes no
store: numpy byte matrices.  Every comparison is an exact equality; every output has guard bytes behind it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.haplotypes_reference import (  # noqa: E402
    ALL_COMPLETE, SYMBOL_NONE, complete_rows, haplotype_ids, mask_of, padded_rows, position_symbols,
)
from tests.test_grouped_kernels_gpu import (  # noqa: E402
    LAYOUT_IDS, LAYOUTS, LISTED_POSITIONS, N_ROWS, POSITIONS, _alphabet, _assert_layout, _layout_store, _matrix,
)
from tests.test_kernels_gpu import NUC_CHARS, make_store  # noqa: E402

FILL = 0xA5
GUARD = 16
TWELVE = LISTED_POSITIONS + [5, 1, 2, 12, 22, 7]  # the six kinds of position, one of them once more, and six others


def _split(got, k, rows):
    """(the columns [k][rows], the guard bytes behind them)"""
    return got[:k * rows].reshape(k, rows), got[k * rows:]


def test_the_listed_columns_exercise_every_override_pass():
    assert len(TWELVE) == 12 and len(set(TWELVE)) == 11 and max(TWELVE) < POSITIONS
    for alphabet in ("nuc", "aa"):
        table = _alphabet(alphabet)
        sym = _matrix(alphabet)
        columns = sym[:, LISTED_POSITIONS]
        valid = set(table.valid_mutation_symbols)
        whole = (sym == table.missing).all(axis=1)
        assert whole.sum() > 100                                        # rows that are missing throughout
        assert ((columns == table.missing) & ~whole[:, None]).any(axis=0).all()  # the missing symbol inside runs of other rows
        ambiguity = ~np.isin(columns, list(valid)) & (columns != table.missing)
        assert ambiguity.any(axis=0).all()                              # ambiguity codes (sparse keys) in every listed column
        assert all(len(valid & set(np.unique(columns[:, c]).tolist())) > 1 for c in range(columns.shape[1]))  # more than one valid symbol


@pytest.mark.parametrize("knob4,knob8", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("alphabet", ["nuc", "aa"])
def test_symbol_columns_in_every_layout(built, alphabet, knob4, knob8):
    sym = _matrix(alphabet)
    store = _layout_store(alphabet, knob4, knob8)
    try:
        _assert_layout(store, alphabet, knob4, knob8)
        rows = store.row_words * 64
        assert rows == padded_rows(N_ROWS)
        for listed in (LISTED_POSITIONS, TWELVE):
            k = len(listed)
            got, unresolved, status = store.position_symbols(0, listed, fill=FILL, guard_bytes=GUARD)
            assert status == 0
            columns, guard = _split(got, k, rows)
            want = position_symbols(sym, listed, rows)
            assert np.array_equal(columns[:, :N_ROWS], want[:, :N_ROWS]), (alphabet, knob4, knob8, listed)
            assert (columns[:, N_ROWS:] == SYMBOL_NONE).all()           # the padding rows
            assert unresolved[0] == 0                                   # every cell of a real row has a symbol
            assert (guard == FILL).all() and (unresolved[1:] == 0xA5A5A5A5).all()
            twice, unresolved_twice, status = store.position_symbols(0, listed, fill=FILL, guard_bytes=GUARD, calls=2)
            assert status == 0 and np.array_equal(twice, got) and np.array_equal(unresolved_twice, unresolved)
    finally:
        store.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("positions", [1, 3])
def test_small_stores(built, n, positions):
    """Rows around a word, a 256-byte line and the row padding of 2 048; a run of the missing symbol that starts at position 0, one
    that ends at the last position, an ambiguity code in the last real row."""
    table = _alphabet("nuc")
    rng = np.random.default_rng(100 * n + positions)
    sym = rng.integers(0, 5, size=(n, positions)).astype(np.uint8)
    sym[0, 0:max(1, positions - 1)] = table.missing          # starts at position 0
    sym[n // 2, min(1, positions - 1):positions] = table.missing  # ends at P
    sym[n - 1, positions - 1] = 6                              # Y in the last real row
    store = make_store(n, [dict(name="a", alphabet="nuc", reference=np.full(positions, 1, dtype=np.uint8))])
    try:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        rows = store.row_words * 64
        assert rows == padded_rows(n)
        for listed in ([0], list(range(positions))[::-1], [positions - 1, 0, positions - 1]):
            got, unresolved, status = store.position_symbols(0, listed, fill=FILL, guard_bytes=GUARD)
            columns, guard = _split(got, len(listed), rows)
            assert status == 0 and np.array_equal(columns, position_symbols(sym, listed, rows)), (n, positions, listed)
            assert unresolved[0] == 0 and (guard == FILL).all() and (unresolved[1:] == 0xA5A5A5A5).all()
    finally:
        store.close()


@pytest.mark.parametrize("k", [1, 5, 6, 7, 12])
@pytest.mark.parametrize("n_symbols,valid", [(16, [0, 1, 2, 3, 4]), (25, list(range(21)) + [23])], ids=["nuc", "aa"])
def test_tuple_ids_and_the_row_bitset(built, k, n_symbols, valid):
    from silo_amd import binding

    rng = np.random.default_rng(1000 * k + n_symbols)
    row_words = 33                      # no multiple of a block's 4 words: the last block is partial
    rows = row_words * 64
    sequence_count = rows - 70          # the padding begins inside a word
    symbols = rng.integers(0, n_symbols, size=(k, rows)).astype(np.uint8)
    symbols[:, ::3] = rng.choice(valid, size=symbols[:, ::3].shape)  # rows of valid symbols only, so that some are complete
    symbols[rng.integers(0, k, size=40), rng.integers(0, rows, size=40)] = SYMBOL_NONE
    symbols[:, sequence_count:] = SYMBOL_NONE
    symbols[0, sequence_count + 3] = 1  # whatever the padding rows hold: their ids are 0, their bits clear
    filter_words = rng.integers(0, 2**63, size=row_words, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=row_words, dtype=np.uint64)
    filter_words[-2:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # stray bits past sequence_count
    want_ids = haplotype_ids(symbols, sequence_count, n_symbols)
    assert len(np.unique(want_ids[:, :sequence_count], axis=1).T) > min(sequence_count // 2, n_symbols ** min(k, 6) // 2)
    for complete in (mask_of(valid), ALL_COMPLETE):
        for words in (filter_words, None):
            ids, row_bits, status = binding.haplotype_ids(symbols, sequence_count, n_symbols, complete, words, fill=FILL, guard_words=4)
            assert status == 0 and ids.shape == ((k + 5) // 6, rows + 4)
            assert np.array_equal(ids[:, :rows], want_ids), (k, n_symbols)
            want_bits = complete_rows(symbols, sequence_count, complete, words)
            assert np.array_equal(row_bits[:row_words], want_bits), (k, n_symbols, complete)
            selected = sum(bin(int(w)).count("1") for w in want_bits)
            assert 0 < selected < sequence_count or (words is None and complete == ALL_COMPLETE and selected == sequence_count)
            assert int(row_bits[row_words - 1]) == 0 and int(row_bits[row_words - 2]) >> (64 - 6) == 0  # the 70 padding bits
            assert (ids[:, rows:] == 0xA5A5A5A5).all() and (row_bits[row_words:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    ids, row_bits, status = binding.haplotype_ids(symbols, sequence_count, n_symbols, want_rows=False, fill=FILL, guard_words=4)
    assert status == 0 and row_bits is None and np.array_equal(ids[:, :rows], want_ids)


def test_refusals_leave_the_fill(built):
    from silo_amd import binding

    table = _alphabet("nuc")
    sym = np.random.default_rng(5).integers(0, 5, size=(100, 4)).astype(np.uint8)
    sym[7, 1:3] = table.missing
    store = make_store(100, [dict(name="a", alphabet="nuc", reference=sym[0].copy())])
    unfinished = make_store(100, [dict(name="a", alphabet="nuc", reference=sym[0].copy())])
    try:
        store.append_sequences(0, 0, NUC_CHARS[sym])
        store.finalize()
        unfinished.append_sequences(0, 0, NUC_CHARS[sym])
        cases = [(store, 0, [0, 1], dict(null=("store",))), (store, 0, [0, 1], dict(null=("positions",))), (store, 0, [0, 1], dict(null=("symbols",))),
                 (store, 0, [0, 1], dict(null=("unresolved",))), (store, 1, [0, 1], {}), (store, 0, [0, 4], {}), (store, 0, [0xFFFFFFFF], {}),
                 (store, 0, [0, 1], dict(n_positions=0)), (store, 0, list(range(4)) * 3 + [0], {}), (unfinished, 0, [0, 1], {})]
        for target, seqstore_id, listed, options in cases:
            got, unresolved, status = target.position_symbols(seqstore_id, listed, fill=FILL, guard_bytes=GUARD, **options)
            assert status != 0 and (got == FILL).all() and (unresolved == 0xA5A5A5A5).all(), (seqstore_id, listed, options)
        got, unresolved, status = store.position_symbols(0, list(range(4)) * 3, fill=FILL)  # the most positions, each listed three times
        assert status == 0 and unresolved[0] == 0 and np.array_equal(got.reshape(12, -1), position_symbols(sym, list(range(4)) * 3))
    finally:
        store.close()
        unfinished.close()

    symbols = np.zeros((7, 128), dtype=np.uint8)
    refused = [dict(null=("symbols",)), dict(null=("ids",)), dict(null=("column",)), dict(n_symbols=0), dict(n_symbols=33), dict(n_positions=0),
               dict(n_positions=13), dict(row_words=0), dict(sequence_count=129)]
    for options in refused:
        arguments = dict(dict(sequence_count=100, n_symbols=16, fill=FILL, guard_words=2), **options)
        ids, row_bits, status = binding.haplotype_ids(symbols, **arguments)
        assert status != 0 and (ids == 0xA5A5A5A5).all() and (row_bits == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), options
    ids, row_bits, status = binding.haplotype_ids(symbols, 128, 32, fill=FILL)  # the limits themselves are taken
    assert status == 0 and not ids.any() and (row_bits == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
