"""MutationsPerSequence / AminoAcidMutationsPerSequence: what each selected sequence carries against the reference — substitutions,
runs of deletions and of the missing symbol, ambiguous positions — from the gathered rows and the differences kernel (K18), through
JSON and the engine: against the numpy reference of tests/sequence_differences_reference.py applied to the strings the oracle's
FastaAligned returns for the same filter, against the engine's own FastaAligned and Mutations rows, and on synthetic stores in every
adaptive layout against the reference on the raw symbol matrix.  Every comparison is an exact equality.

The numbers that the tests assert of the reference before they compare (main = the default nucleotide sequence, 29 903 positions; S =
the gene, 1 274) were worked out on the CPU with the oracle; tests/test_sequence_differences_reference.py asserts them without a GPU.
Main's 4 786 words are more than the 32 x 100 of the first call: the second runs.  S's 1 777 are fewer: it does not."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dataset  # noqa: E402
from tests.pair_distances_reference import NUC_CHARS, NUC_VALID  # noqa: E402
from tests.sequence_differences_reference import COUNT_FIELDS, FIRST_WORDS_PER_ROW, LIST_FIELDS, MAX_ROWS, difference_records, response_rows  # noqa: E402
from tests.test_consensus_gpu import _chars, _reference_of  # noqa: E402  (the cache of the oracle's strings is shared)
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

KEY = "gisaid_epi_isl"
FIELDS = {KEY, "sequenceName", *LIST_FIELDS, *COUNT_FIELDS}
ORDERABLE = [KEY, *COUNT_FIELDS]
SEQUENCES = [(None, "main", "nuc"), ("S", "S", "aa")]  # (sequenceName of the request, the store, its alphabet)
TOTALS = {"main": (4786, [3033, 6691, 60723, 35]), "S": (1777, [1371, 1667, 3031, 0])}  # words and cells of the four kinds, all 100 rows
TRUE = {"type": "True"}
FALSE = {"type": "False"}


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


def _action(sequence_name, alphabet, **fields):
    action = dict(fields, type="MutationsPerSequence" if alphabet == "nuc" else "AminoAcidMutationsPerSequence")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _filters(data):
    return [(TRUE, 100), (LINEAGE, 51), (_key_is(data, 40, 3, 99, 57, 38), 5), (_key_is(data, 5, 30, 36, 0), 4), (_key_is(data, 37), 1), (FALSE, 0)]


def _want(oracle_db, data, store, alphabet, expression):
    keys, chars = _chars(oracle_db, store, expression)
    return response_rows(keys, chars, _reference_of(data, store, alphabet), alphabet, store, KEY)


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        chars = _chars(oracle_db, store, TRUE)[1]
        offsets, stats, words = difference_records(chars, _reference_of(data, store, alphabet), alphabet)
        assert (len(words), stats.sum(axis=0).tolist()) == TOTALS[store]  # the reference itself
        assert (len(words) > FIRST_WORDS_PER_ROW * 100) == (store == "main")  # the second call runs on main only
        for expression, selects in _filters(data):
            want = _want(oracle_db, data, store, alphabet, expression)
            assert len(want) == selects, (store, expression)
            got = engine.execute_query({"action": _action(sequence_name, alphabet), "filterExpression": expression})
            assert got == want, (store, expression, [(a, b) for a, b in zip(got, want) if a != b][:1])
            assert all(set(row) == FIELDS for row in got)
        everything = engine.execute_query({"action": _action(sequence_name, alphabet), "filterExpression": TRUE})
        assert [sum(row[field] for row in everything) for field in COUNT_FIELDS] == TOTALS[store][1]
        assert [row[KEY] for row in everything] == data["keys"]  # partition order, then ascending row id


def test_the_reference_on_the_engines_own_fasta_aligned_rows_gives_the_same_response(example):
    engine, _, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        for expression, selects in _filters(data):
            aligned = engine.execute_query({"action": {"type": "FastaAligned", "sequenceName": store}, "filterExpression": expression})
            assert len(aligned) == selects
            chars = np.array([list(row[store].encode()) for row in aligned], dtype=np.uint8).reshape(len(aligned), len(_reference_of(data, store, alphabet)))
            want = response_rows([row[KEY] for row in aligned], chars, _reference_of(data, store, alphabet), alphabet, store, KEY)
            assert engine.execute_query({"action": _action(sequence_name, alphabet), "filterExpression": expression}) == want, (store, expression)


def _positions_of(runs):
    """The 1-based positions of a deletions / missing field."""
    for run in runs.split(",") if runs else []:
        first, _, last = run.partition("-")
        yield from range(int(first), int(last or first) + 1)


def test_the_rows_that_carry_a_mutation_are_as_many_as_mutations_counts(example):
    engine, _, data = example
    for sequence_name, store, alphabet in SEQUENCES:
        reference = _reference_of(data, store, alphabet)
        for expression, selects in _filters(data):
            got = engine.execute_query({"action": _action(sequence_name, alphabet), "filterExpression": expression})
            carried = collections.Counter()
            for row in got:
                carried.update(row["substitutions"].split(",") if row["substitutions"] else [])
                carried.update(f"{reference[p - 1]}{p}-" for p in _positions_of(row["deletions"]))
            mutations = engine.execute_query({"action": {"type": "Mutations" if alphabet == "nuc" else "AminoAcidMutations", "sequenceName": store, "minProportion": 0},
                                              "filterExpression": expression})
            assert {row["mutation"]: row["count"] for row in mutations} == dict(carried), (store, expression)  # every Mutations row accounted for
            assert len(mutations) == len(carried) and (len(carried) > 0) == (selects > 0)


def test_order_limit_offset(example):
    engine, _, _ = example
    for sequence_name, _, alphabet in SEQUENCES:
        base = _action(sequence_name, alphabet)
        got = engine.execute_query({"action": base, "filterExpression": TRUE})
        assert len(got) == 100
        unique = sorted(got, key=lambda row: row[KEY])
        for field in ORDERABLE:
            for descending in (False, True):
                order_by = [{"field": field, "order": "descending" if descending else "ascending"}, KEY]
                want = sorted(unique, key=lambda row: row[field], reverse=descending)  # (stable, reversed or not: ties stay by key)
                for limit, offset in ((4, 2), (10_000, 0), (5, 97)):
                    ordered = engine.execute_query({"action": dict(base, orderByFields=order_by, limit=limit, offset=offset), "filterExpression": TRUE})
                    assert ordered == want[offset:offset + limit], (field, descending, limit, offset)
            assert len({row[field] for row in got}) >= 3 or (alphabet, field) == ("aa", "ambiguousPositions")  # something to put in order
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": TRUE}) == got[2:6]  # the default order
        assert engine.execute_query({"action": dict(base, offset=100), "filterExpression": TRUE}) == []


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _ = example
    ok = {"type": "MutationsPerSequence"}
    gene = {"type": "AminoAcidMutationsPerSequence", "sequenceName": "S"}
    cases = [
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName=None), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "Database does not contain a sequence with name: 'nosuchsequence'"),
        (dict(ok, sequenceName="S"), "'S'"),  # a gene is no nucleotide sequence
        ({"type": "AminoAcidMutationsPerSequence"}, "sequenceName"),
        (dict(gene, sequenceName="main"), "'main'"),
        (dict(gene, sequenceName=["S"]), "sequenceName"),
        (dict(ok, orderByFields=["sequenceName"]), "OrderByField sequenceName is not contained in the result of this operation."),
        (dict(ok, orderByFields=["substitutions"]), "OrderByField substitutions"),
        (dict(gene, orderByFields=[{"field": "deletions", "order": "ascending"}]), "OrderByField deletions"),
        (dict(ok, orderByFields=["main"]), "OrderByField main"),
        (dict(ok, limit=-1), "limit"),
        (dict(ok, offset="2"), "offset"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (ok, dict(ok, sequenceName="main"), dict(ok, sequenceName="testSecondSequence", orderByFields=ORDERABLE), gene,
                   dict(gene, sequenceName="ORF1a", orderByFields=ORDERABLE)):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and len(document["queryResult"]) == 51 and all(set(row) == FIELDS for row in document["queryResult"]), document
        assert {row["sequenceName"] for row in document["queryResult"]} == {action.get("sequenceName", "main")}


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        for action in ({"type": "MutationsPerSequence"}, {"type": "AminoAcidMutationsPerSequence", "sequenceName": "S"}):
            status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
            assert status == 400 and "sharded" in document["message"] and action["type"] in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2028)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


_SYNTHETIC_WANT = {}  # selection number -> the rows wanted


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the rows gathered from derived symbols, runs of N, sparse ambiguity keys and code planes, then the
    differences, for a stretch of 3 001 rows, the 9 999 and 10 000 rows up to the limit, scattered rows of a bucket and no row; one
    row more than the limit and the whole store are refused."""
    sym, _, bucket = synthetic
    reference = "".join(NUC_VALID[1 + (p % 4)] for p in range(POSITIONS))  # as _synthetic_engine gives it
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    rows = np.arange(N_ROWS)
    selections = [
        ({"type": "IntBetween", "column": "row", "from": 30_000, "to": 33_000}, (rows >= 30_000) & (rows <= 33_000)),
        ({"type": "IntBetween", "column": "row", "from": 130_004, "to": N_ROWS}, rows >= 130_004),
        ({"type": "IntBetween", "column": "row", "from": 3, "to": MAX_ROWS + 2}, (rows >= 3) & (rows <= MAX_ROWS + 2)),
        ({"type": "IntEquals", "column": "bucket", "value": 7}, bucket == 7),
        (FALSE, np.zeros(N_ROWS, dtype=bool)),
    ]
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        sizes = []
        for number, (expression, mask) in enumerate(selections):
            if number not in _SYNTHETIC_WANT:  # the same for every layout: worked out once
                selected = np.flatnonzero(mask)
                _SYNTHETIC_WANT[number] = response_rows([str(row) for row in selected], lut[sym[selected]], reference, "nuc", "main", "key")
            want = _SYNTHETIC_WANT[number]
            got = engine.execute_query({"action": {"type": "MutationsPerSequence"}, "filterExpression": expression})
            assert got == want, (layout, missing_runs, expression, [(a, b) for a, b in zip(got, want) if a != b][:1])
            sizes.append(len(want))
        assert sizes[:3] == [3001, MAX_ROWS - 1, MAX_ROWS] and 50 < sizes[3] < 400 and sizes[4] == 0
        assert all(any(row[field] for row in _SYNTHETIC_WANT[0]) for field in COUNT_FIELDS) and any(row["missing"] == "1-48" for row in _SYNTHETIC_WANT[2])
        for expression in (TRUE, {"type": "IntBetween", "column": "row", "from": 3, "to": MAX_ROWS + 3}):
            status, document = engine.execute_raw({"action": {"type": "MutationsPerSequence"}, "filterExpression": expression})
            assert status == 400 and "MutationsPerSequence action currently limited to 10000 sequences" in document["message"], document
    finally:
        engine.close()
