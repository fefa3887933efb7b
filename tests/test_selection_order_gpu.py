"""The order of the selected rows, which FastaAligned, MutationsPerSequence and the distance actions all take from one walk over the
selection: partition order, then ascending row id.  A synthetic database of 100 rows in three partitions (37, 1 and 62 rows) with a
nucleotide sequence of 29 positions and a gene of 11; the primary keys are a permutation of the rows, so that no ordering by key gives
the order asserted.  Every comparison is an exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARTITION_SIZES = [37, 1, 62]
N_ROWS = sum(PARTITION_SIZES)
NUC_CHARS, AA_CHARS = "-ACGTRYSWKMBDHVN", "-ACDEFGHIKLMNPQRSTVWYBZ*X"
POSITIONS, GENE_LENGTH = 29, 11
TRUE = {"type": "True"}
FALSE = {"type": "False"}
# nothing of the one-row partition (row 37); rows of the first and of the third partition
SOME = {"type": "Or", "children": [{"type": "IntBetween", "column": "row", "from": 30, "to": 36}, {"type": "IntEquals", "column": "row", "value": 5},
                                   {"type": "IntBetween", "column": "row", "from": 38, "to": 45}, {"type": "IntEquals", "column": "row", "value": 99}]}
SOME_ROWS = [5, *range(30, 37), *range(38, 46), 99]


def _strings(rng, chars, length):
    lut = np.frombuffer(chars.encode(), dtype=np.uint8)
    return [bytes(row).decode() for row in lut[rng.integers(0, len(chars), size=(N_ROWS, length))]]


@pytest.fixture(scope="module")
def store(built):
    from silo_amd.engine import Engine

    rng = np.random.default_rng(2031)
    main, gene = _strings(rng, NUC_CHARS, POSITIONS), _strings(rng, AA_CHARS, GENE_LENGTH)
    keys = [f"k{(row * 37) % N_ROWS:02d}" for row in range(N_ROWS)]  # a permutation: 37 and 100 are coprime
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": "ACGT" * 7 + "A"}], "genes": [{"name": "S", "sequence": "MFVFLVLLPLV"}]})
    engine.set_schema("key")
    first = 0
    for size in PARTITION_SIZES:
        part = engine.add_partition(size)
        engine.append_sequences(part, "main", False, 0, main[first:first + size])
        engine.append_sequences(part, "S", True, 0, gene[first:first + size])
        engine.append_metadata(part, "key", "string", keys[first:first + size])
        engine.append_metadata(part, "row", "int", [str(row) for row in range(first, first + size)])
        first += size
    engine.finalize()
    yield engine, keys, main, gene
    engine.close()


def _query(engine, action, expression):
    return engine.execute_query({"action": action, "filterExpression": expression})


@pytest.mark.parametrize("expression,rows", [(TRUE, list(range(N_ROWS))), (SOME, SOME_ROWS)], ids=["every-row", "no-row-of-the-one-row-partition"])
def test_the_three_families_number_the_selection_by_partition_then_row(store, expression, rows):
    engine, keys, main, gene = store
    assert len(set(keys)) == N_ROWS and sorted(rows) == rows and rows[0] < 37 < rows[-1] and (37 in rows) == (expression is TRUE)
    selected = [keys[row] for row in rows]
    assert selected != sorted(selected) and selected != sorted(selected, reverse=True)  # the order is not one of the keys

    aligned = _query(engine, {"type": "FastaAligned", "sequenceName": ["main", "S"]}, expression)
    assert aligned == [{"key": keys[row], "main": main[row], "S": gene[row]} for row in rows]

    for action, name in (({"type": "MutationsPerSequence"}, "main"), ({"type": "AminoAcidMutationsPerSequence", "sequenceName": "S"}, "S")):
        per_sequence = _query(engine, action, expression)
        assert [row["key"] for row in per_sequence] == selected
        assert {row["sequenceName"] for row in per_sequence} == {name}

    for sequence_name in ("main", "S"):
        pairs = _query(engine, {"type": "DistanceMatrix", "sequenceName": sequence_name}, expression)  # no orderByFields
        assert [(row["firstKey"], row["secondKey"]) for row in pairs] == [(selected[i], selected[j]) for i in range(len(rows)) for j in range(i + 1, len(rows))]


def test_a_filter_that_selects_nothing_gives_no_rows(store):
    engine = store[0]
    for action in ({"type": "FastaAligned", "sequenceName": ["main", "S"]}, {"type": "MutationsPerSequence"},
                   {"type": "AminoAcidMutationsPerSequence", "sequenceName": "S"}, {"type": "DistanceMatrix"}, {"type": "DistanceMatrix", "sequenceName": "S"}):
        assert _query(engine, action, FALSE) == []
