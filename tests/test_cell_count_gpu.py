"""CellCount, the filter expression that bounds a row's number of substitutions, deletions, missing or ambiguous cells, and
CellCountDistribution, the histogram of that number (K22), through JSON and the engine: on the example data set as one partition and
as three against two oracles — numpy (tests/cell_counts_reference.py) on the strings the oracle's FastaAligned returns, and the
engine's own MutationsPerSequence rows, which share no kernel with K22 — and on the 140 003 x 48 synthetic stores in every adaptive
layout against numpy on the raw symbol matrix.  Every comparison is an exact equality.

The gene S of the example data set holds no ambiguity code: the kind "ambiguous" is constant there, so S is not used for it; a copy
of the data set with planted codes (planted_data) is, against numpy on the planted strings and MutationsPerSequence.
tests/test_cell_counts_reference.py checks on the CPU that every threshold and every binning used here cuts its fixture."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cell_counts_reference as ref  # noqa: E402
from tests import dataset  # noqa: E402
from tests import distinct_reference  # noqa: E402
from tests import sample_reference  # noqa: E402
from tests.test_cell_count_parse import SHARDED, UNKNOWN_SEQUENCE  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, PARTITION_SIZES, _build_example_engine, _key_is, _tuned_engine  # noqa: E402
from tests.test_distance_matrix_gpu import example, example_data, synthetic  # noqa: E402,F401  (fixtures)
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS  # noqa: E402
from tests.test_nearest_neighbours_gpu import _strings  # noqa: E402
from tests.test_within_distance_gpu import _check_selection, _count_of, _keys_of, _mask_words  # noqa: E402

KEY = "gisaid_epi_isl"
EVERYTHING = {"type": "True"}
NO_BOUND = 0xFFFFFFFF
COUNT_FIELDS = ("substitutionCount", "deletedPositions", "missingPositions", "ambiguousPositions")
# (sequenceName, alphabet, kinds) on the example data set: every single kind and a list per sequence, but no ambiguity codes in S
EXAMPLE_CASES = [(None, "nuc", kinds) for kinds in ("substitutions", "deletions", "missing", "ambiguous", ["missing", "ambiguous"], list(ref.KINDS))] + \
                [("S", "aa", kinds) for kinds in ("substitutions", "deletions", "missing", ["substitutions", "deletions"])]
PLANTED_CASES = [("S", "aa", "ambiguous"), ("S", "aa", ["ambiguous", "missing"])]
PLANTED_CODES = {4: 3, 38: 1, 70: 2, 99: 1}  # row -> ambiguity codes planted in its gene S
# (sequenceName, alphabet, kinds, binWidth, maxBins) of the distributions
EXAMPLE_BINNINGS = [(None, "nuc", "missing", 100, 8), (None, "nuc", "substitutions", 1, None), (None, "nuc", ["ambiguous"], 1, 3),
                    ("S", "aa", ["substitutions", "deletions"], 5, 4), (None, "nuc", list(ref.KINDS), 64, 4096)]
PLANTED_BINNINGS = [("S", "aa", "ambiguous", 1, None), ("S", "aa", "ambiguous", 2, 2)]
SYNTHETIC_KINDS = ["substitutions", "deletions", "missing", "ambiguous", ["substitutions", "missing"]]
SYNTHETIC_BINNINGS = [("missing", 1, None), (["substitutions", "missing"], 4, 10)]  # (kinds, binWidth, maxBins)


def cell_count(kinds, sequence_name=None, **bounds):
    expression = dict(bounds, type="CellCount", cells=kinds)
    if sequence_name is not None:
        expression["sequenceName"] = sequence_name
    return expression


def distribution(kinds, sequence_name=None, **fields):
    action = dict({k: v for k, v in fields.items() if v is not None}, type="CellCountDistribution", cells=kinds)
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def bounds_for(value):
    """The bounds a test asks for, from the values present: at most the median, at least one above it, both quartiles, the maximum
    alone, 0 to the median — (atLeast, atMost), None = absent."""
    ordered = np.sort(np.asarray(value))
    median, low, high = int(ordered[len(ordered) // 2]), int(ordered[len(ordered) // 4]), int(ordered[3 * len(ordered) // 4])
    return [(None, median), (median + 1, None), (low, high), (int(ordered[-1]), None), (0, median)]


def mask_for(value, at_least, at_most):
    value = np.asarray(value)
    return (value >= (0 if at_least is None else at_least)) & (value <= (NO_BOUND if at_most is None else at_most))


def with_bounds(kinds, sequence_name, at_least, at_most):
    bounds = {name: bound for name, bound in (("atLeast", at_least), ("atMost", at_most)) if bound is not None}
    return cell_count(kinds, sequence_name, **bounds)


def table_of_strings(strings, references, sequence_name, alphabet):
    """uint32 [rows][4] of aligned strings (None: no genome) against the reference of the sequence."""
    reference = references[sequence_name or "main"]
    chars, missing = (ref.NUC, "N") if alphabet == "nuc" else (ref.AA, "X")
    sym = distinct_reference.symbols_of_strings(strings, chars, missing, len(reference))
    return ref.cells(sym, distinct_reference.symbols_of_strings([reference], chars, missing, len(reference))[0], alphabet)


@functools.lru_cache(maxsize=None)
def example_table(sequence_name, alphabet):
    """The cell counts of the example data set from its own files: what the CPU guard sees (the GPU tests take the oracle's strings
    and assert that they give this table)."""
    data = dataset.load_example_dataset()
    strings = data["nuc" if alphabet == "nuc" else "aa"][sequence_name or "main"]
    return table_of_strings(strings, data["nuc_references" if alphabet == "nuc" else "aa_references"], sequence_name, alphabet)


@functools.lru_cache(maxsize=None)
def planted_data():
    """The example data set with ambiguity codes (B, Z) planted in the gene S of four rows, one of them the last row."""
    data = dict(dataset.load_example_dataset())
    data["aa"] = {name: list(rows) for name, rows in data["aa"].items()}
    rows = data["aa"]["S"]
    for row, codes in PLANTED_CODES.items():
        text = list(rows[row])
        at = [p for p in range(len(text)) if text[p] in "DNEQ"][:codes]
        assert len(at) == codes
        for p in at:
            text[p] = "B" if text[p] in "DN" else "Z"
        rows[row] = "".join(text)
    return data


@functools.lru_cache(maxsize=None)
def planted_table(sequence_name, alphabet):
    data = planted_data()
    strings = data["nuc" if alphabet == "nuc" else "aa"][sequence_name or "main"]
    return table_of_strings(strings, data["nuc_references" if alphabet == "nuc" else "aa_references"], sequence_name, alphabet)


def _oracle_table(oracle_db, data, sequence_name, alphabet):
    """The first oracle: numpy on the strings of the oracle's FastaAligned, in the order of the data set."""
    strings = dict(_strings(oracle_db, sequence_name, EVERYTHING))
    references = data["nuc_references" if alphabet == "nuc" else "aa_references"]
    table = table_of_strings([strings[key] for key in data["keys"]], references, sequence_name, alphabet)
    assert np.array_equal(table, example_table(sequence_name, alphabet))
    return table


def _per_sequence_table(engine, data, sequence_name, alphabet):
    """The second oracle: the four counts of the engine's MutationsPerSequence rows, in the order of the data set."""
    action = {"type": "MutationsPerSequence"} if alphabet == "nuc" else {"type": "AminoAcidMutationsPerSequence", "sequenceName": sequence_name}
    rows = {row[KEY]: [row[field] for field in COUNT_FIELDS] for row in engine.execute_query({"action": action, "filterExpression": EVERYTHING})}
    return np.array([rows[key] for key in data["keys"]], dtype=np.uint32)


def _check_cases(engine, data, partition_sizes, cases, table_of):
    for sequence_name, alphabet, kinds in cases:
        table = table_of(sequence_name, alphabet)
        assert np.array_equal(table, _per_sequence_table(engine, data, sequence_name, alphabet)), (sequence_name, "the two oracles differ")
        value = ref.values(table, ref.mask_of(kinds))
        for at_least, at_most in bounds_for(value):
            expression = with_bounds(kinds, sequence_name, at_least, at_most)
            _check_selection(engine, data, partition_sizes, expression, mask_for(value, at_least, at_most), (sequence_name, kinds, at_least, at_most))


def test_example_dataset_matches_both_oracles(example):
    engine, oracle_db, data, partition_sizes = example
    _check_cases(engine, data, partition_sizes, EXAMPLE_CASES, lambda name, alphabet: _oracle_table(oracle_db, data, name, alphabet))
    # the default nucleotide sequence by its name
    value = ref.values(example_table(None, "nuc"), ref.MISSING)
    _check_selection(engine, data, partition_sizes, cell_count("missing", "main", atMost=100), value <= 100, "main by name")


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def planted(request, built):
    engine = _build_example_engine(planted_data(), request.param)
    yield engine, planted_data(), request.param
    engine.close()


def test_ambiguity_codes_of_a_gene_on_planted_data(planted):
    engine, data, partition_sizes = planted
    _check_cases(engine, data, partition_sizes, PLANTED_CASES, planted_table)
    ambiguous = planted_table("S", "aa")[:, 3]
    assert {row: int(ambiguous[row]) for row in np.flatnonzero(ambiguous)} == PLANTED_CODES
    _check_selection(engine, data, partition_sizes, cell_count("ambiguous", "S", atLeast=2), ambiguous >= 2, "planted rows")


def test_composition_with_other_expressions(example):
    engine, _, data, partition_sizes = example
    n = len(data["keys"])
    lineage_keys = _keys_of(engine, LINEAGE)
    lineage = np.array([key in lineage_keys for key in data["keys"]])
    missing = ref.values(example_table(None, "nuc"), ref.MISSING)
    changed = ref.values(example_table("S", "aa"), ref.SUBSTITUTIONS | ref.DELETIONS)
    first, second = missing <= 100, changed >= 10
    a, b = cell_count("missing", atMost=100), cell_count(["substitutions", "deletions"], "S", atLeast=10)
    assert (first & lineage).any() and (first & ~lineage).any() and (first != second).any() and second.any() and (~first).any()
    votes = first.astype(int) + second + lineage
    cases = [
        ({"type": "And", "children": [a, LINEAGE]}, first & lineage),
        ({"type": "And", "children": [LINEAGE, {"type": "Not", "child": a}]}, lineage & ~first),
        ({"type": "Or", "children": [a, b]}, first | second),
        ({"type": "And", "children": [a, b]}, first & second),
        ({"type": "Not", "child": a}, ~first),
        ({"type": "Not", "child": {"type": "Or", "children": [a, b]}}, ~(first | second)),
        ({"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [a, b, LINEAGE]}, votes >= 2),
        ({"type": "N-Of", "numberOfMatchers": 1, "matchExactly": True, "children": [a, b, LINEAGE]}, votes == 1),
        ({"type": "Maybe", "child": a}, first),   # the ambiguity mode is ignored
        ({"type": "Exact", "child": b}, second),
        ({"type": "Not", "child": {"type": "Maybe", "child": b}}, ~second),
    ]
    for expression, mask in cases:
        _check_selection(engine, data, partition_sizes, expression, mask, expression["type"])
    # under DistinctSequences and Sample, and with those as siblings
    sym = distinct_reference.symbols_of_strings(data["nuc"]["main"], ref.NUC, "N", len(data["nuc_references"]["main"]))
    everything = np.ones(n, dtype=bool)
    distinct_all, sampled = distinct_reference.select(sym, everything), sample_reference.select(4, 40, everything)
    nested = [
        ({"type": "DistinctSequences", "child": a}, distinct_reference.select(sym, first)),
        ({"type": "Sample", "child": a, "size": 7, "seed": 2}, sample_reference.select(2, 7, first)),
        ({"type": "And", "children": [a, {"type": "DistinctSequences", "child": EVERYTHING}]}, first & distinct_all),
        ({"type": "And", "children": [{"type": "Not", "child": a}, {"type": "Sample", "child": EVERYTHING, "size": 40, "seed": 4}]}, ~first & sampled),
    ]
    assert 0 < sample_reference.select(2, 7, first).sum() == 7 and (~first & sampled).any()
    for expression, mask in nested:
        _check_selection(engine, data, partition_sizes, expression, mask, ("nested", expression["type"]))


def test_mutations_under_the_expression_equal_those_under_its_keys(example):
    engine, _, data, _ = example
    rows = np.flatnonzero(ref.values(example_table(None, "nuc"), ref.MISSING) <= 100)
    assert 2 < len(rows) < len(data["keys"])
    for action in ({"type": "Mutations", "minProportion": 0.05, "orderByFields": ["mutation"]},
                   {"type": "AminoAcidMutations", "sequenceName": "S", "minProportion": 0.05, "orderByFields": ["mutation"]}):
        got = engine.execute_query({"action": action, "filterExpression": cell_count("missing", atMost=100)})
        want = engine.execute_query({"action": action, "filterExpression": _key_is(data, *rows)})
        assert got == want and got, action["type"]


def test_compile_answers_without_the_table(built, example_data):
    """Full, Empty and the empty selection of the action leave every store as it is (its device bytes do not grow); the first
    query that needs the table adds 16 bytes per padded row, a second one nothing."""
    engine = _build_example_engine(example_data, None)
    try:
        n = len(example_data["keys"])
        positions = len(example_data["nuc_references"]["main"])
        before = engine.partition_store(0).device_bytes
        shortcuts = [(cell_count("missing", atLeast=0, atMost=positions), n), (cell_count("missing", atMost=positions + 5), n), (cell_count("missing", atMost=NO_BOUND), n),
                     (cell_count(list(ref.KINDS), atLeast=0), n), (cell_count("missing", atLeast=positions + 1), 0), (cell_count("deletions", atLeast=8, atMost=7), 0),
                     (cell_count("missing", atLeast=NO_BOUND), 0), ({"type": "Not", "child": cell_count("ambiguous", atLeast=0)}, 0)]
        for expression, count in shortcuts:
            assert _count_of(engine, expression) == count, expression
        assert engine.execute_query({"action": distribution("missing"), "filterExpression": {"type": "False"}}) == []
        assert engine.execute_query({"action": distribution("missing"), "filterExpression": cell_count("missing", atLeast=positions + 1)}) == []
        assert engine.partition_store(0).device_bytes == before
        value = ref.values(example_table(None, "nuc"), ref.MISSING)
        assert _count_of(engine, cell_count("missing", atLeast=positions)) == int((value >= positions).sum())  # not decided by the positions alone
        rows = engine.partition_store(0).row_words * 64
        assert engine.partition_store(0).device_bytes == before + 16 * rows
        assert _count_of(engine, cell_count("deletions", atMost=30)) == int((example_table(None, "nuc")[:, 1] <= 30).sum())
        assert engine.execute_query({"action": distribution("missing", binWidth=100), "filterExpression": EVERYTHING})
        assert engine.partition_store(0).device_bytes == before + 16 * rows
        assert _count_of(engine, cell_count("missing", "S", atMost=0)) == int((example_table("S", "aa")[:, 2] == 0).sum())  # another sequence store
        assert engine.partition_store(0).device_bytes == before + 32 * rows
    finally:
        engine.close()


def test_batch_of_counts_answers_as_single_queries(example):
    engine, _, data, _ = example
    filters = [
        cell_count("missing", atMost=100),
        {"type": "And", "children": [LINEAGE, cell_count("substitutions", "S", atLeast=10)]},
        cell_count(["ambiguous", "missing"], atLeast=1, atMost=50),
        {"type": "Not", "child": cell_count("deletions", atMost=30)},
        LINEAGE,
        cell_count("missing", atLeast=0),
    ]
    queries = [{"action": {"type": "Aggregated"}, "filterExpression": expression} for expression in filters]
    singles = [engine.execute_query(query) for query in queries]
    batch = engine.execute_batch(queries)
    assert [status for status, _ in batch] == [200] * 6
    assert [document["queryResult"] for _, document in batch] == singles
    table = example_table(None, "nuc")
    assert singles[0][0]["count"] == int((table[:, 2] <= 100).sum()) and singles[3][0]["count"] == int((table[:, 1] > 30).sum())
    assert singles[5][0]["count"] == len(data["keys"]) and len({single[0]["count"] for single in singles}) > 3


def _check_distributions(engine, data, binnings, table_of):
    lineage_keys = _keys_of(engine, LINEAGE)
    lineage = np.array([key in lineage_keys for key in data["keys"]])
    for sequence_name, alphabet, kinds, bin_width, max_bins in binnings:
        table = table_of(sequence_name, alphabet)
        for expression, rows in ((EVERYTHING, np.ones(len(table), dtype=bool)), (LINEAGE, lineage)):
            want = ref.response_rows(ref.bins(table, rows, ref.mask_of(kinds), bin_width, max_bins or 1024), bin_width)
            got = engine.execute_query({"action": distribution(kinds, sequence_name, binWidth=bin_width, maxBins=max_bins), "filterExpression": expression})
            assert got == want, (sequence_name, kinds, bin_width, max_bins, expression["type"])
            assert sum(row["count"] for row in got) == _count_of(engine, expression) == int(rows.sum())
            assert all(set(row) == {"from", "to", "count"} for row in got)


def test_distribution_matches_numpy(example):
    engine, _, data, _ = example
    _check_distributions(engine, data, EXAMPLE_BINNINGS, example_table)
    # the open last bin, the default binWidth and maxBins
    got = engine.execute_query({"action": distribution("missing", binWidth=100, maxBins=8), "filterExpression": EVERYTHING})
    assert got[-1]["from"] == 700 and got[-1]["to"] is None and got[0] == {"from": 0, "to": 99, "count": got[0]["count"]}
    default = engine.execute_query({"action": distribution("substitutions"), "filterExpression": EVERYTHING})
    assert all(row["to"] == row["from"] for row in default) and len(default) > 10


def test_distribution_on_planted_data(planted):
    engine, data, _ = planted
    _check_distributions(engine, data, PLANTED_BINNINGS, planted_table)


def test_distribution_order_limit_offset(example):
    engine, _, _, _ = example
    base = distribution("substitutions", binWidth=2)
    got = engine.execute_query({"action": base, "filterExpression": EVERYTHING})
    assert [row["from"] for row in got] == sorted(row["from"] for row in got) and len(got) > 8
    in_python = sorted(got, key=lambda row: (-row["count"], row["from"]))
    assert in_python != got
    for limit, offset in ((4, 2), (1000, 0), (3, len(got) - 2)):
        ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "count", "order": "descending"}, "from"], limit=limit, offset=offset),
                                        "filterExpression": EVERYTHING})
        assert ordered == in_python[offset:offset + limit]
    assert engine.execute_query({"action": dict(base, limit=3, offset=1), "filterExpression": EVERYTHING}) == got[1:4]
    descending = engine.execute_query({"action": dict(base, orderByFields=[{"field": "from", "order": "descending"}]), "filterExpression": EVERYTHING})
    assert descending == got[::-1]
    status, document = engine.execute_raw({"action": dict(base, orderByFields=["to"]), "filterExpression": EVERYTHING})
    assert status == 400 and document["message"] == "OrderByField to is not contained in the result of this operation.", document


def test_unknown_sequences_are_bad_requests(example):
    engine, _, _, _ = example
    for query, message in (
        ({"action": {"type": "Aggregated"}, "filterExpression": cell_count("missing", "nosuchsequence", atMost=3)}, UNKNOWN_SEQUENCE.format("CellCount", "nosuchsequence")),
        ({"action": {"type": "Aggregated"}, "filterExpression": {"type": "Not", "child": cell_count("missing", "nosuchsequence", atMost=3)}},
         UNKNOWN_SEQUENCE.format("CellCount", "nosuchsequence")),
        ({"action": distribution("missing", "nosuchsequence"), "filterExpression": EVERYTHING}, UNKNOWN_SEQUENCE.format("CellCountDistribution", "nosuchsequence")),
    ):
        status, document = engine.execute_raw(query)
        assert status == 400 and document["error"] == "Bad request" and document["message"] == message, document


@pytest.mark.parametrize("by_position", [False, True], ids=["sequence-shard", "position-shard"])
def test_sharded_engine_refuses(built, example_data, by_position):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, by_position)
        status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": cell_count("missing", atMost=100)})
        assert status == 400 and document["message"] == SHARDED["CellCount"], document
        status, document = engine.execute_raw({"action": distribution("missing"), "filterExpression": EVERYTHING})
        assert status == 400 and document["message"] == SHARDED["CellCountDistribution"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
_SYNTHETIC_TABLE = []


def synthetic_table(sym):
    """The cell counts of the synthetic matrix against the synthetic engines' reference (computed once, never changed)."""
    if not _SYNTHETIC_TABLE:
        table = ref.cells(sym, 1 + np.arange(POSITIONS) % 4, "nuc")
        table.setflags(write=False)
        _SYNTHETIC_TABLE.append(table)
    return _SYNTHETIC_TABLE[0]


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):  # noqa: F811
    """140 003 rows x 48 positions: the filter for every kind and the action under all rows and a scattered selection."""
    sym, _, bucket = synthetic
    table = synthetic_table(sym)
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for kinds in SYNTHETIC_KINDS:
            value = ref.values(table, ref.mask_of(kinds))
            for at_least, at_most in bounds_for(value)[:3]:
                want = mask_for(value, at_least, at_most)
                expression = with_bounds(kinds, None, at_least, at_most)
                words, count = engine.evaluate_filter(expression, partition=0, n_rows=N_ROWS)
                assert np.array_equal(words, _mask_words(want)), (layout, missing_runs, kinds, at_least, at_most)
                assert count == int(want.sum()), (layout, missing_runs, kinds, at_least, at_most)
        scattered = {"type": "IntBetween", "column": "bucket", "from": 0, "to": 99}
        for kinds, bin_width, max_bins in SYNTHETIC_BINNINGS:
            for expression, rows in ((EVERYTHING, np.ones(N_ROWS, dtype=bool)), (scattered, bucket < 100)):
                want = ref.response_rows(ref.bins(table, rows, ref.mask_of(kinds), bin_width, max_bins or 1024), bin_width)
                got = engine.execute_query({"action": distribution(kinds, binWidth=bin_width, maxBins=max_bins), "filterExpression": expression})
                assert got == want and len(got) > 1, (layout, missing_runs, kinds, expression["type"])
        few = engine.execute_query({"action": {"type": "Details", "fields": ["key"]}, "filterExpression": cell_count("missing", atLeast=POSITIONS)})
        assert sorted(int(row["key"]) for row in few) == np.flatnonzero(table[:, 2] == POSITIONS).tolist() and len(few) > 100
    finally:
        engine.close()
