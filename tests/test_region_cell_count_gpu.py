"""CellCount over a position range (positionFrom / positionTo) and the action CellCountByRegion (K23), through JSON and the engine:
on the example data set as one partition and as three against two oracles — numpy (tests/region_counts_reference.py) on the strings
the oracle's FastaAligned returns, and the positions counted out of the engine's own MutationsPerSequence rows, which share no kernel
with K23 — and on the 140 003 x 48 synthetic stores in every adaptive layout against numpy on the raw symbol matrix.  Every
comparison is an exact equality.  tests/test_region_counts_reference.py checks on the CPU that every threshold used here cuts its
fixture and that the action's counts are not all 0 or all of the selection."""
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cell_counts_reference as whole  # noqa: E402
from tests import dataset  # noqa: E402
from tests import distinct_reference  # noqa: E402
from tests import region_counts_reference as ref  # noqa: E402
from tests import sample_reference  # noqa: E402
from tests.test_cell_count_gpu import cell_count, example_table, mask_for  # noqa: E402
from tests.test_cell_count_parse import UNKNOWN_SEQUENCE  # noqa: E402
from tests.test_distance_matrix_gpu import LINEAGE, PARTITION_SIZES, _build_example_engine, _key_is, _tuned_engine  # noqa: E402
from tests.test_distance_matrix_gpu import example, example_data, synthetic  # noqa: E402,F401  (fixtures)
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS  # noqa: E402
from tests.test_nearest_neighbours_gpu import _strings  # noqa: E402
from tests.test_region_cell_count_parse import FROM_PAST_THE_END, PAST_THE_END, REGION_PAST_THE_END, SHARDED  # noqa: E402
from tests.test_within_distance_gpu import _check_selection, _count_of, _keys_of, _mask_words  # noqa: E402

KEY = "gisaid_epi_isl"
EVERYTHING = {"type": "True"}
NO_BOUND = 0xFFFFFFFF
MAIN_POSITIONS, S_POSITIONS = 29903, 1274
# 1-based inclusive regions: the genes' coordinates on the SARS-CoV-2 reference, single positions, both ends, the whole sequence
MAIN_REGIONS = {"ORF1a": (266, 13468), "S": (21563, 25384), "E": (26245, 26472), "M": (26523, 27191), "N": (28274, 29533), "first": (1, 1),
                "last": (MAIN_POSITIONS, MAIN_POSITIONS), "241": (241, 241), "23403": (23403, 23403), "whole": (1, MAIN_POSITIONS), "first100": (1, 100)}
S_REGIONS = {"NTD": (14, 305), "RBD": (319, 541), "614": (614, 614), "first": (1, 1), "last": (S_POSITIONS, S_POSITIONS), "whole": (1, S_POSITIONS),
             "S2": (686, S_POSITIONS)}
# (sequenceName, alphabet, kinds, region): every kind, every region; no kind is constant on its region (the CPU guard checks)
EXAMPLE_CASES = [
    (None, "nuc", "substitutions", "ORF1a"), (None, "nuc", "missing", "S"), (None, "nuc", "missing", "E"), (None, "nuc", "missing", "M"),
    (None, "nuc", ["substitutions", "deletions"], "N"), (None, "nuc", "ambiguous", "ORF1a"), (None, "nuc", "deletions", "S"), (None, "nuc", "missing", "first"),
    (None, "nuc", "deletions", "last"), (None, "nuc", "substitutions", "23403"), (None, "nuc", ["substitutions", "deletions"], "241"),
    (None, "nuc", list(whole.KINDS), "whole"), (None, "nuc", "missing", "first100"),
    ("S", "aa", "substitutions", "RBD"), ("S", "aa", "missing", "NTD"), ("S", "aa", "substitutions", "614"), ("S", "aa", "deletions", "first"),
    ("S", "aa", "deletions", "last"), ("S", "aa", ["substitutions", "deletions"], "whole"), ("S", "aa", "missing", "S2"),
]
# CellCountByRegion on main: 16 amplicon-like regions of 400 positions that overlap their neighbours by 100, and the genes, shuffled;
# "mostly N" is a bound of each region's own, "complete coverage" the action's
AMPLICONS = [("amplicon %d" % k, 31 + 300 * k, 430 + 300 * k) for k in range(16)]
GENES = [(name, *MAIN_REGIONS[name]) for name in ("S", "ORF1a", "E", "N", "M")]


def action_regions():
    """[(name, from, to, atLeast or None, atMost or None)] in a shuffled request order."""
    regions = [(name, first, last, (last - first + 1) // 2 if k % 2 else None, None) for k, (name, first, last) in enumerate(AMPLICONS + GENES)]
    order = np.random.default_rng(41).permutation(len(regions))
    return [regions[g] for g in order]


def many_regions():
    """256 regions of 100 positions, each overlapping the next by half: two colours."""
    return [("r%03d" % k, 1 + 50 * k, 100 + 50 * k, None, None) for k in range(ref.MAX_REGIONS)]


def region_count(kinds, region, sequence_name=None, **bounds):
    """The expression for a 1-based inclusive region (first, last); None leaves the field out."""
    expression = cell_count(kinds, sequence_name, **bounds)
    for field, position in zip(("positionFrom", "positionTo"), region):
        if position is not None:
            expression[field] = position
    return expression


def by_region(kinds, regions, sequence_name=None, **fields):
    action = dict(fields, type="CellCountByRegion", cells=kinds, regions=[
        dict({"name": name, "positionFrom": first, "positionTo": last}, **{k: v for k, v in (("atLeast", low), ("atMost", high)) if v is not None})
        for name, first, last, low, high in regions])
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def region_bounds(value):
    """(atLeast, atMost) pairs cut from the values present: below a middle value, from it on, exactly it.  None = absent."""
    present = np.unique(np.asarray(value))
    assert len(present) >= 2
    middle = int(present[len(present) // 2])
    return [(None, middle - 1), (middle, None), (middle, middle)]


def with_bounds(kinds, region, sequence_name, at_least, at_most):
    return region_count(kinds, region, sequence_name, **{name: bound for name, bound in (("atLeast", at_least), ("atMost", at_most)) if bound is not None})


def symbols_of(strings, references, sequence_name, alphabet):
    """(sym [rows][P], reference [P]) of aligned strings."""
    reference = references[sequence_name or "main"]
    chars, missing = (whole.NUC, "N") if alphabet == "nuc" else (whole.AA, "X")
    sym = distinct_reference.symbols_of_strings(strings, chars, missing, len(reference))
    return sym, distinct_reference.symbols_of_strings([reference], chars, missing, len(reference))[0]


@functools.lru_cache(maxsize=None)
def example_symbols(sequence_name, alphabet):
    """The example data set from its own files: what the CPU guard sees (the GPU tests assert that the oracle's strings give it)."""
    data = dataset.load_example_dataset()
    strings = data["nuc" if alphabet == "nuc" else "aa"][sequence_name or "main"]
    return symbols_of(strings, data["nuc_references" if alphabet == "nuc" else "aa_references"], sequence_name, alphabet)


def example_value(sequence_name, alphabet, kinds, region):
    """uint32 [rows]: the first oracle's value for a 1-based inclusive region."""
    sym, reference = example_symbols(sequence_name, alphabet)
    return ref.values(sym, reference, alphabet, [(region[0] - 1, region[1])], whole.mask_of(kinds))[0]


def action_counts(regions, value_of, rows, at_least=None, at_most=None):
    """The counts of a CellCountByRegion: value_of(first, last) is the value of every row, a region's own bounds replace the action's."""
    counts = []
    for _, first, last, low, high in regions:
        if low is None and high is None:
            low, high = at_least, at_most
        counts.append(int((mask_for(value_of(first, last), low, high) & rows).sum()))
    return counts


_ORACLE_CHECKED = set()


def _oracle_value(oracle_db, data, sequence_name, alphabet, kinds, region):
    """The first oracle: numpy on the strings of the oracle's FastaAligned, in the order of the data set."""
    if (sequence_name, alphabet) not in _ORACLE_CHECKED:
        strings = dict(_strings(oracle_db, sequence_name, EVERYTHING))
        sym, _ = symbols_of([strings[key] for key in data["keys"]], data["nuc_references" if alphabet == "nuc" else "aa_references"], sequence_name, alphabet)
        assert np.array_equal(sym, example_symbols(sequence_name, alphabet)[0])
        _ORACLE_CHECKED.add((sequence_name, alphabet))
    return example_value(sequence_name, alphabet, kinds, region)


def _per_sequence_classes(engine, data, sequence_name, alphabet):
    """The second oracle: uint8 [rows][P], 1 + kind of every cell that MutationsPerSequence lists (0: the reference's symbol)."""
    positions = MAIN_POSITIONS if alphabet == "nuc" else S_POSITIONS
    action = {"type": "MutationsPerSequence"} if alphabet == "nuc" else {"type": "AminoAcidMutationsPerSequence", "sequenceName": sequence_name}
    rows = {row[KEY]: row for row in engine.execute_query({"action": action, "filterExpression": EVERYTHING})}
    classes = np.zeros((len(data["keys"]), positions), dtype=np.uint8)
    for r, key in enumerate(data["keys"]):
        for k, kind in enumerate(whole.KINDS):
            for item in filter(None, rows[key][kind].split(",")):
                if k in (1, 2):  # deletions, missing: "5" or "5-30"
                    first, _, last = item.partition("-")
                    span = slice(int(first) - 1, int(last or first))
                else:            # substitutions, ambiguous: "C241T"
                    position = int(re.fullmatch(r".(\d+).", item).group(1))
                    span = slice(position - 1, position)
                assert not classes[r, span].any()
                classes[r, span] = k + 1
    return classes


def _value_of_classes(classes, kinds, region):
    mask = whole.mask_of(kinds)
    inside = np.isin(classes[:, region[0] - 1:region[1]], [k + 1 for k in range(4) if (mask >> k) & 1])
    return inside.sum(axis=1).astype(np.uint32)


def test_example_dataset_matches_both_oracles(example):
    engine, oracle_db, data, partition_sizes = example
    classes = {}
    for sequence_name, alphabet, kinds, region_name in EXAMPLE_CASES:
        region = (MAIN_REGIONS if alphabet == "nuc" else S_REGIONS)[region_name]
        value = _oracle_value(oracle_db, data, sequence_name, alphabet, kinds, region)
        if (sequence_name, alphabet) not in classes:
            classes[sequence_name, alphabet] = _per_sequence_classes(engine, data, sequence_name, alphabet)
        assert np.array_equal(value, _value_of_classes(classes[sequence_name, alphabet], kinds, region)), (sequence_name, region_name, "the two oracles differ")
        for at_least, at_most in region_bounds(value):
            expression = with_bounds(kinds, region, sequence_name, at_least, at_most)
            _check_selection(engine, data, partition_sizes, expression, mask_for(value, at_least, at_most), (sequence_name, kinds, region_name, at_least, at_most))
    # an absent positionFrom is 1, an absent positionTo the sequence's length; the default nucleotide sequence by its name
    value = example_value(None, "nuc", "missing", (1, 100))
    _check_selection(engine, data, partition_sizes, region_count("missing", (None, 100), "main", atLeast=1), value >= 1, "positionTo alone")
    value = example_value(None, "nuc", "missing", (29804, MAIN_POSITIONS))
    _check_selection(engine, data, partition_sizes, region_count("missing", (29804, None), atLeast=1), value >= 1, "positionFrom alone")


def test_the_whole_sequence_gives_the_rows_of_the_expression_without_a_region(example):
    engine, _, data, partition_sizes = example
    for sequence_name, alphabet, kinds, positions in ((None, "nuc", "missing", MAIN_POSITIONS), ("S", "aa", ["substitutions", "deletions"], S_POSITIONS)):
        value = whole.values(example_table(sequence_name, alphabet), whole.mask_of(kinds))
        assert np.array_equal(value, example_value(sequence_name, alphabet, kinds, (1, positions)))
        for at_least, at_most in region_bounds(value):
            bounds = {name: bound for name, bound in (("atLeast", at_least), ("atMost", at_most)) if bound is not None}
            for region in ((1, positions), (None, positions), (1, None)):
                expression = region_count(kinds, region, sequence_name, **bounds)
                assert _keys_of(engine, expression) == _keys_of(engine, cell_count(kinds, sequence_name, **bounds)), (sequence_name, region)
            _check_selection(engine, data, partition_sizes, region_count(kinds, (1, positions), sequence_name, **bounds), mask_for(value, at_least, at_most), sequence_name)


def test_composition_with_other_expressions(example):
    engine, _, data, partition_sizes = example
    n = len(data["keys"])
    lineage_keys = _keys_of(engine, LINEAGE)
    lineage = np.array([key in lineage_keys for key in data["keys"]])
    covered = example_value(None, "nuc", "missing", MAIN_REGIONS["S"])
    changed = example_value("S", "aa", "substitutions", S_REGIONS["RBD"])
    first, second = covered <= 0, changed >= 3
    a = region_count("missing", MAIN_REGIONS["S"], atMost=0)                       # complete coverage of the spike gene
    b = region_count("substitutions", S_REGIONS["RBD"], "S", atLeast=3)            # at least 3 substitutions in the receptor-binding domain
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
        ({"type": "Not", "child": {"type": "Maybe", "child": b}}, ~second),
    ]
    for expression, mask in cases:
        _check_selection(engine, data, partition_sizes, expression, mask, expression["type"])
    sym = example_symbols(None, "nuc")[0]
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
    rows = np.flatnonzero(example_value(None, "nuc", "missing", MAIN_REGIONS["S"]) == 0)
    assert 2 < len(rows) < len(data["keys"])
    for action in ({"type": "Mutations", "minProportion": 0.05, "orderByFields": ["mutation"]},
                   {"type": "AminoAcidMutations", "sequenceName": "S", "minProportion": 0.05, "orderByFields": ["mutation"]}):
        got = engine.execute_query({"action": action, "filterExpression": region_count("missing", MAIN_REGIONS["S"], atMost=0)})
        want = engine.execute_query({"action": action, "filterExpression": _key_is(data, *rows)})
        assert got == want and got, action["type"]


def test_compile_answers_without_the_store_and_a_region_keeps_nothing(built, example_data):
    """Full and Empty, decided by the region's length, and the empty selection of the action leave every store as it is; so does a
    query that does count a region; the whole sequence as a region builds the kept table of the expression without one."""
    engine = _build_example_engine(example_data, None)
    try:
        n = len(example_data["keys"])
        before = engine.partition_store(0).device_bytes
        gene = MAIN_REGIONS["E"]  # 228 positions
        shortcuts = [(region_count("missing", gene, atLeast=0, atMost=228), n), (region_count("missing", gene, atMost=300), n),
                     (region_count(list(whole.KINDS), (5, 5), atLeast=0, atMost=1), n), (region_count("missing", gene, atLeast=229), 0),
                     (region_count("missing", (5, 5), atLeast=2), 0), (region_count("deletions", gene, atLeast=8, atMost=7), 0),
                     ({"type": "Not", "child": region_count("ambiguous", gene, atLeast=0)}, 0)]
        for expression, count in shortcuts:
            assert _count_of(engine, expression) == count, expression
        regions = [("E", *gene, None, None), ("S", *MAIN_REGIONS["S"], 5, None)]
        empty = engine.execute_query({"action": by_region("missing", regions, atMost=0), "filterExpression": {"type": "False"}})
        assert empty == ref.response_rows(["E", "S"], [(gene[0] - 1, gene[1]), (21562, 25384)], [0, 0], 0)
        assert engine.partition_store(0).device_bytes == before
        value = example_value(None, "nuc", "missing", gene)
        assert _count_of(engine, region_count("missing", gene, atLeast=228)) == int((value >= 228).sum())  # not decided by the length alone
        assert _count_of(engine, region_count("missing", gene, atMost=0)) == int((value == 0).sum()) and 0 < int((value == 0).sum()) < n
        assert engine.execute_query({"action": by_region("missing", regions, atMost=0), "filterExpression": EVERYTHING})
        assert engine.partition_store(0).device_bytes == before  # nothing is kept of a region
        rows = engine.partition_store(0).row_words * 64
        whole_value = whole.values(example_table(None, "nuc"), whole.MISSING)
        assert _count_of(engine, region_count("missing", (1, MAIN_POSITIONS), atMost=100)) == int((whole_value <= 100).sum())
        assert engine.partition_store(0).device_bytes == before + 16 * rows  # the kept table of K22
        assert _count_of(engine, cell_count("missing", atMost=100)) == int((whole_value <= 100).sum())
        assert engine.partition_store(0).device_bytes == before + 16 * rows
    finally:
        engine.close()


def test_batch_of_counts_answers_as_single_queries(example):
    engine, _, data, _ = example
    filters = [
        region_count("missing", MAIN_REGIONS["S"], atMost=0),
        {"type": "And", "children": [LINEAGE, region_count("substitutions", S_REGIONS["RBD"], "S", atLeast=3)]},
        region_count(["substitutions", "deletions"], MAIN_REGIONS["241"], atLeast=1),
        {"type": "Not", "child": region_count("deletions", MAIN_REGIONS["S"], atMost=0)},
        LINEAGE,
        region_count("missing", MAIN_REGIONS["E"], atLeast=0),
    ]
    queries = [{"action": {"type": "Aggregated"}, "filterExpression": expression} for expression in filters]
    singles = [engine.execute_query(query) for query in queries]
    batch = engine.execute_batch(queries)
    assert [status for status, _ in batch] == [200] * 6
    assert [document["queryResult"] for _, document in batch] == singles
    assert singles[0][0]["count"] == int((example_value(None, "nuc", "missing", MAIN_REGIONS["S"]) == 0).sum())
    assert singles[3][0]["count"] == int((example_value(None, "nuc", "deletions", MAIN_REGIONS["S"]) > 0).sum())
    assert singles[5][0]["count"] == len(data["keys"]) and len({single[0]["count"] for single in singles}) > 3


def _example_action_rows(regions, rows, kinds="missing", sequence_name=None, alphabet="nuc", at_least=None, at_most=None):
    counts = action_counts(regions, lambda first, last: example_value(sequence_name, alphabet, kinds, (first, last)), rows, at_least, at_most)
    return ref.response_rows([region[0] for region in regions], [(region[1] - 1, region[2]) for region in regions], counts, int(rows.sum()))


def test_action_with_overlapping_regions_in_shuffled_order(example):
    engine, _, data, _ = example
    lineage_keys = _keys_of(engine, LINEAGE)
    lineage = np.array([key in lineage_keys for key in data["keys"]])
    regions = action_regions()
    for expression, rows in ((EVERYTHING, np.ones(len(lineage), dtype=bool)), (LINEAGE, lineage)):
        got = engine.execute_query({"action": by_region("missing", regions, atMost=0), "filterExpression": expression})
        assert got == _example_action_rows(regions, rows, at_most=0), expression["type"]
        assert all(set(row) == {"region", "positionFrom", "positionTo", "count", "total"} for row in got)
        assert {row["total"] for row in got} == {_count_of(engine, expression)} == {int(rows.sum())}
        assert any(0 < row["count"] < row["total"] for row in got)
    # an amino-acid gene, the action's bounds alone, every kind
    s_regions = [(name, first, last, None, None) for name, (first, last) in S_REGIONS.items()]
    got = engine.execute_query({"action": by_region(["substitutions", "deletions"], s_regions, "S", atLeast=1, atMost=20), "filterExpression": EVERYTHING})
    assert got == _example_action_rows(s_regions, np.ones(len(lineage), dtype=bool), ["substitutions", "deletions"], "S", "aa", 1, 20)
    assert any(0 < row["count"] < row["total"] for row in got)


def test_action_with_256_regions(example):
    engine, _, data, _ = example
    regions = many_regions()
    rows = np.ones(len(data["keys"]), dtype=bool)
    got = engine.execute_query({"action": by_region(["missing", "deletions"], regions, atLeast=1), "filterExpression": EVERYTHING})
    assert got == _example_action_rows(regions, rows, ["missing", "deletions"], at_least=1) and len(got) == ref.MAX_REGIONS
    assert len({row["count"] for row in got}) > 3


def test_action_order_limit_offset(example):
    engine, _, _, _ = example
    base = by_region("missing", action_regions(), atMost=0)
    got = engine.execute_query({"action": base, "filterExpression": EVERYTHING})
    assert [row["region"] for row in got] == [region[0] for region in action_regions()]  # request order
    in_python = sorted(got, key=lambda row: (-row["count"], row["region"]))
    assert in_python != got
    for limit, offset in ((4, 2), (1000, 0), (3, len(got) - 2)):
        ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "count", "order": "descending"}, "region"], limit=limit, offset=offset),
                                        "filterExpression": EVERYTHING})
        assert ordered == in_python[offset:offset + limit]
    assert engine.execute_query({"action": dict(base, limit=3, offset=1), "filterExpression": EVERYTHING}) == got[1:4]
    by_position = engine.execute_query({"action": dict(base, orderByFields=["positionFrom", {"field": "positionTo", "order": "descending"}]), "filterExpression": EVERYTHING})
    assert by_position == sorted(got, key=lambda row: (row["positionFrom"], -row["positionTo"]))
    status, document = engine.execute_raw({"action": dict(base, orderByFields=["total"]), "filterExpression": EVERYTHING})
    assert status == 400 and document["message"] == "OrderByField total is not contained in the result of this operation.", document


def test_positions_past_the_end_and_unknown_sequences_are_bad_requests(example):
    engine, _, _, _ = example
    aggregated = {"type": "Aggregated"}
    region = [("a", 10, MAIN_POSITIONS + 1, None, None)]
    for query, message in (
        ({"action": aggregated, "filterExpression": region_count("missing", (5, MAIN_POSITIONS + 1), atMost=3)}, PAST_THE_END.format(MAIN_POSITIONS + 1, "main", MAIN_POSITIONS)),
        ({"action": aggregated, "filterExpression": region_count("missing", (None, 1275), "S", atMost=3)}, PAST_THE_END.format(1275, "S", S_POSITIONS)),
        ({"action": aggregated, "filterExpression": {"type": "Not", "child": region_count("missing", (1, 40000), atLeast=0)}}, PAST_THE_END.format(40000, "main", MAIN_POSITIONS)),
        ({"action": aggregated, "filterExpression": region_count("missing", (MAIN_POSITIONS + 1, None), atMost=3)},
         FROM_PAST_THE_END.format(MAIN_POSITIONS + 1, "main", MAIN_POSITIONS)),
        ({"action": aggregated, "filterExpression": region_count("missing", (1, 5), "nosuchsequence", atMost=3)}, UNKNOWN_SEQUENCE.format("CellCount", "nosuchsequence")),
        ({"action": by_region("missing", region, atMost=0), "filterExpression": EVERYTHING}, REGION_PAST_THE_END.format("a", MAIN_POSITIONS + 1, "main", MAIN_POSITIONS)),
        ({"action": by_region("missing", region, atMost=0), "filterExpression": {"type": "False"}}, REGION_PAST_THE_END.format("a", MAIN_POSITIONS + 1, "main", MAIN_POSITIONS)),
        ({"action": by_region("missing", [("a", 1, 5, None, None)], "nosuchsequence", atMost=0), "filterExpression": EVERYTHING},
         UNKNOWN_SEQUENCE.format("CellCountByRegion", "nosuchsequence")),
    ):
        status, document = engine.execute_raw(query)
        assert status == 400 and document["error"] == "Bad request" and document["message"] == message, document
    # the last position is inside
    assert _count_of(engine, region_count("missing", (MAIN_POSITIONS, MAIN_POSITIONS), atLeast=0, atMost=1)) == 100


@pytest.mark.parametrize("by_position", [False, True], ids=["sequence-shard", "position-shard"])
def test_sharded_engine_refuses(built, example_data, by_position):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, by_position)
        status, document = engine.execute_raw({"action": {"type": "Aggregated"}, "filterExpression": region_count("missing", MAIN_REGIONS["S"], atMost=0)})
        assert status == 400 and document["message"] == SHARDED["CellCount"], document
        status, document = engine.execute_raw({"action": by_region("missing", [("S", *MAIN_REGIONS["S"], None, None)], atMost=0), "filterExpression": EVERYTHING})
        assert status == 400 and document["message"] == SHARDED["CellCountByRegion"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
SYNTHETIC_REGIONS = [(1, POSITIONS), (1, 1), (POSITIONS, POSITIONS), (5, 30), (17, 17), (31, POSITIONS)]  # 1-based inclusive
SYNTHETIC_KINDS = ["substitutions", "deletions", "missing", "ambiguous", ["substitutions", "missing"]]
SYNTHETIC_ACTION = [("late", 25, POSITIONS, None, None), ("early", 1, 24, 2, None), ("middle", 13, 36, None, 0), ("one", 17, 17, 1, 1), ("all", 1, POSITIONS, 3, 20)]
_SYNTHETIC_CELLS = {}


def synthetic_value(sym, kinds, region):
    """The value of the synthetic matrix against the synthetic engines' reference (the region's cells computed once, never changed)."""
    if region not in _SYNTHETIC_CELLS:
        cells = ref.region_cells(sym, 1 + np.arange(POSITIONS) % 4, "nuc", [(region[0] - 1, region[1])])
        cells.setflags(write=False)
        _SYNTHETIC_CELLS[region] = cells
    return ref.values_of_cells(_SYNTHETIC_CELLS[region], whole.mask_of(kinds))[0]


def synthetic_cases(sym):
    """(kinds, region, atLeast, atMost) for every kind whose value varies on a region: the first two of region_bounds."""
    for region in SYNTHETIC_REGIONS:
        for kinds in SYNTHETIC_KINDS:
            value = synthetic_value(sym, kinds, region)
            if len(np.unique(value)) >= 2:
                for at_least, at_most in region_bounds(value)[:2]:
                    yield kinds, region, at_least, at_most


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):  # noqa: F811
    """140 003 rows x 48 positions: the filter for every kind and region and the action under all rows and a scattered selection."""
    sym, _, bucket = synthetic
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for kinds, region, at_least, at_most in synthetic_cases(sym):
            want = mask_for(synthetic_value(sym, kinds, region), at_least, at_most)
            expression = with_bounds(kinds, region, None, at_least, at_most)
            words, count = engine.evaluate_filter(expression, partition=0, n_rows=N_ROWS)
            assert np.array_equal(words, _mask_words(want)), (layout, missing_runs, kinds, region, at_least, at_most)
            assert count == int(want.sum()), (layout, missing_runs, kinds, region, at_least, at_most)
        scattered = {"type": "IntBetween", "column": "bucket", "from": 0, "to": 99}
        for kinds in ("missing", ["substitutions", "ambiguous"]):
            for expression, rows in ((EVERYTHING, np.ones(N_ROWS, dtype=bool)), (scattered, bucket < 100)):
                counts = action_counts(SYNTHETIC_ACTION, lambda first, last: synthetic_value(sym, kinds, (first, last)), rows, 1, None)
                want = ref.response_rows([region[0] for region in SYNTHETIC_ACTION], [(region[1] - 1, region[2]) for region in SYNTHETIC_ACTION], counts, int(rows.sum()))
                got = engine.execute_query({"action": by_region(kinds, SYNTHETIC_ACTION, atLeast=1), "filterExpression": expression})
                assert got == want, (layout, missing_runs, kinds, expression["type"])
    finally:
        engine.close()
