"""Haplotypes / AminoAcidHaplotypes: the combinations of symbols at listed positions among the rows a filter selects, and their
counts, from the symbol columns of K16 and the group-by of Aggregated, through JSON and the engine: against the numpy reference of
tests/haplotypes_reference.py applied to the strings the oracle's FastaAligned returns, against the engine's own Aggregated under
And(filter, symbol equals ...), and on synthetic stores in every adaptive layout against the reference on the raw symbol matrix.
Every comparison is an exact equality (a proportion is one IEEE division of two integers on either side).

The positions are chosen here, on the CPU, from the oracle's strings, so that the reference alone shows at least three distinct
haplotypes, one that contains the missing symbol and one that contains '-'; each is asserted of the reference before comparing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dataset  # noqa: E402
from tests.haplotypes_reference import haplotype_rows  # noqa: E402
from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_consensus_gpu import _chars  # noqa: E402
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, POSITIONS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

TRUE = {"type": "True"}
FALSE = {"type": "False"}
SEQUENCES = [(None, "main", NUC_CHARS, NUC_VALID, "N"), ("S", "S", AA_CHARS, AA_VALID, "X")]  # (sequenceName, store, alphabet, valid, missing)


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


def _action(sequence_name, positions, **fields):
    action = dict(fields, type="Haplotypes" if sequence_name is None else "AminoAcidHaplotypes", positions=[p + 1 for p in positions])
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    return action


def _symbols(oracle_db, store, alphabet):
    """(keys, symbol ids uint8 [rows][positions]) of every row, from the oracle's FastaAligned, in the order of the data set."""
    keys, chars = _chars(oracle_db, store, TRUE)
    lookup = np.full(256, 0xFF, dtype=np.uint8)
    lookup[np.frombuffer(alphabet.encode(), dtype=np.uint8)] = np.arange(len(alphabet), dtype=np.uint8)
    sym = lookup[chars]
    assert (sym != 0xFF).all()
    return keys, sym


def _mask(oracle_db, store, keys, expression):
    selected = set(_chars(oracle_db, store, expression)[0])
    return np.array([key in selected for key in keys], dtype=bool)


def _choose_positions(sym, alphabet, missing):
    """Five positions of the matrix, 0-based, not in ascending order: the one with the most distinct symbols, one with '-' in
    some rows, one with the missing symbol in some rows but not all, and two more varied ones."""
    distinct = np.array([len(np.unique(sym[:, p])) for p in range(sym.shape[1])])
    by_variety = [int(p) for p in np.argsort(-distinct, kind="stable")]
    gap, miss = alphabet.index("-"), alphabet.index(missing)
    with_gap = next(p for p in by_variety if (sym[:, p] == gap).any())
    with_missing = next(p for p in by_variety if 0 < (sym[:, p] == miss).sum() < len(sym) and p != with_gap)
    chosen = [by_variety[0], with_gap, with_missing]
    chosen = list(dict.fromkeys(chosen + by_variety))[:5]
    return [chosen[1], chosen[4], chosen[0], chosen[2], chosen[3]]


def _as_dict(rows, fields=()):
    out = {(tuple(row[field] for field in fields), row["haplotype"]): (row["count"], row["proportion"]) for row in rows}
    assert len(out) == len(rows) and all(set(row) == set(fields) | {"haplotype", "count", "proportion"} for row in rows)
    return out


def _want(rows):
    return {(row["groups"], row["haplotype"]): (row["count"], row["proportion"]) for row in rows}


def _metadata(engine, fields):
    """key -> the tuple of the fields' values as the engine renders them (Details: existing code)."""
    rows = engine.execute_query({"action": {"type": "Details", "fields": ["gisaid_epi_isl", *fields]}, "filterExpression": TRUE})
    return {row["gisaid_epi_isl"]: tuple(row[field] for field in fields) for row in rows}


def _count(engine, expression):
    return engine.execute_query({"action": {"type": "Aggregated"}, "filterExpression": expression})[0]["count"]


def _filters(data):
    return [TRUE, LINEAGE, _key_is(data, 37), FALSE]


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data = example
    country = _metadata(engine, ["country"])
    date = _metadata(engine, ["date"])
    division_age = _metadata(engine, ["division", "age"])  # strings and integers, both with nulls
    assert any(value[0] is None for value in division_age.values()) and any(value[1] is None for value in division_age.values())
    for sequence_name, store, alphabet, valid, missing in SEQUENCES:
        keys, sym = _symbols(oracle_db, store, alphabet)
        positions = _choose_positions(sym, alphabet, missing)
        valid_ids = [alphabet.index(c) for c in valid]
        everything = haplotype_rows(sym, positions, alphabet)
        assert len(everything) >= 3, store                                            # the reference itself, before comparing
        assert any(missing in row["haplotype"] for row in everything), store
        assert any("-" in row["haplotype"] for row in everything), store
        assert sum(row["count"] for row in everything) == 100
        for expression in _filters(data):
            mask = _mask(oracle_db, store, keys, expression)
            for exclude in (False, True):
                for fields, values in (((), None), (("country",), country), (("date",), date), (("division", "age"), division_age)):
                    groups = None if values is None else [values[key] for key in keys]
                    want = haplotype_rows(sym, positions, alphabet, mask=mask, valid_symbols=valid_ids if exclude else None, groups=groups)
                    action = _action(sequence_name, positions, excludeIncomplete=exclude, groupByFields=list(fields))
                    got = engine.execute_query({"action": action, "filterExpression": expression})
                    assert _as_dict(got, fields) == _want(want), (store, expression, exclude, fields)
                    if not exclude:
                        assert sum(row["count"] for row in got) == _count(engine, expression) == int(mask.sum())
                    if expression == FALSE:
                        assert got == []
            # excludeIncomplete leaves out exactly the rows the reference says: those with another symbol at a listed position
            complete = np.isin(sym[:, positions], valid_ids).all(axis=1)
            got = engine.execute_query({"action": _action(sequence_name, positions, excludeIncomplete=True), "filterExpression": expression})
            assert sum(row["count"] for row in got) == int((mask & complete).sum())
            if expression == TRUE:
                assert 0 < int(complete.sum()) < 100
        # the default of excludeIncomplete is false, of groupByFields none
        assert _as_dict(engine.execute_query({"action": _action(sequence_name, positions), "filterExpression": LINEAGE})) == _want(
            haplotype_rows(sym, positions, alphabet, mask=_mask(oracle_db, store, keys, LINEAGE)))


def test_every_valid_haplotype_is_an_aggregated_count(example):
    """Parity with existing code: a haplotype of valid symbols only has the count of Aggregated under And(filter, symbol equals ...)."""
    engine, oracle_db, data = example
    for sequence_name, store, alphabet, valid, missing in SEQUENCES:
        _, sym = _symbols(oracle_db, store, alphabet)
        positions = _choose_positions(sym, alphabet, missing)
        for expression in (TRUE, LINEAGE):
            got = engine.execute_query({"action": _action(sequence_name, positions), "filterExpression": expression})
            checked = 0
            for row in got:
                if not all(c in valid for c in row["haplotype"]):
                    continue
                equals = [dict({"type": "NucleotideEquals" if sequence_name is None else "AminoAcidEquals", "position": p + 1, "symbol": c},
                               **({} if sequence_name is None else {"sequenceName": sequence_name})) for p, c in zip(positions, row["haplotype"])]
                assert row["count"] == _count(engine, {"type": "And", "children": [expression, *equals]}), (store, row)
                checked += 1
            assert checked >= 2, store


def test_order_limit_offset(example):
    engine, oracle_db, data = example
    for sequence_name, store, alphabet, _, missing in SEQUENCES:
        _, sym = _symbols(oracle_db, store, alphabet)
        base = _action(sequence_name, _choose_positions(sym, alphabet, missing), groupByFields=["division"])
        got = engine.execute_query({"action": base, "filterExpression": TRUE})
        assert len(got) >= 6 and any(row["division"] is None for row in got)

        def key_of(field):  # a null sorts before every value
            return lambda row: (row[field] is not None, row[field] if row[field] is not None else 0)

        for field in ("division", "haplotype", "count", "proportion"):
            assert len({row[field] for row in got}) >= 2  # something to put in order
            for descending in (False, True):
                order_by = [{"field": field, "order": "descending" if descending else "ascending"}, "haplotype", "division"]
                want = sorted(sorted(got, key=lambda row: (row["haplotype"], key_of("division")(row))), key=key_of(field), reverse=descending)
                for limit, offset in ((4, 2), (1000, 0), (3, len(got) - 2)):
                    ordered = engine.execute_query({"action": dict(base, orderByFields=order_by, limit=limit, offset=offset), "filterExpression": TRUE})
                    assert ordered == want[offset:offset + limit], (store, field, descending)
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": TRUE}) == got[2:6]
        assert engine.execute_query({"action": dict(base, offset=len(got)), "filterExpression": TRUE}) == []
        # the proportions are those of the whole response, whatever limit and offset leave of it
        assert abs(sum(row["proportion"] for row in got) - 1.0) < 1e-9 and all(row["proportion"] == row["count"] / 100 for row in got)


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _ = example
    ok = {"type": "Haplotypes", "positions": [1, 2]}
    cases = [
        ({"type": "Haplotypes"}, "positions"),
        (dict(ok, positions=[]), "positions"),
        (dict(ok, positions=5), "positions"),
        (dict(ok, positions=None), "positions"),
        (dict(ok, positions=list(range(1, 14))), "positions"),
        (dict(ok, positions=list(range(1, 14))), "13"),
        (dict(ok, positions=[3, 7, 3]), "positions"),
        (dict(ok, positions=[3, 7, 3]), "position 3 occurs more than once"),
        (dict(ok, positions=[0]), "positions"),
        (dict(ok, positions=[29904]), "positions"),
        (dict(ok, positions=[29904]), "29904"),
        (dict(ok, positions=[1.5]), "positions"),
        (dict(ok, positions=[-1]), "positions"),
        (dict(ok, positions=["1"]), "positions"),
        (dict(ok, positions=[2**32]), "positions"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "'nosuchsequence'"),
        (dict(ok, sequenceName="S"), "'S'"),  # a gene is no nucleotide sequence
        ({"type": "AminoAcidHaplotypes", "positions": [1]}, "sequenceName"),
        ({"type": "AminoAcidHaplotypes", "positions": [1], "sequenceName": "main"}, "'main'"),
        ({"type": "AminoAcidHaplotypes", "positions": [1275], "sequenceName": "S"}, "positions"),
        (dict(ok, groupByFields=["nosuchfield"]), "'nosuchfield'"),
        (dict(ok, groupByFields=["nosuchfield"]), "groupByFields"),
        (dict(ok, groupByFields="country"), "groupByFields"),
        (dict(ok, groupByFields=[5]), "groupByFields"),
        (dict(ok, groupByFields=["country", "date", "region", "division", "age", "qc_value", "pango_lineage"]), "groupByFields"),
        # 25^12 = 2^55.7 combinations of symbols times more than 2^9 of the five fields: no 64-bit tuple id
        ({"type": "AminoAcidHaplotypes", "sequenceName": "S", "positions": list(range(1, 13)),
          "groupByFields": ["date", "division", "age", "qc_value", "unsorted_date"]}, "2^64 - 1 combinations"),
        (dict(ok, excludeIncomplete="true"), "excludeIncomplete"),
        (dict(ok, excludeIncomplete=1), "excludeIncomplete"),
        (dict(ok, excludeIncomplete=None), "excludeIncomplete"),
        (dict(ok, orderByFields=["gisaid_epi_isl"]), "gisaid_epi_isl"),
        (dict(ok, orderByFields=["country"]), "country"),  # not among the groupByFields
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    fields = ["country", "date", "region", "division", "age", "qc_value"]
    # the limits themselves are taken: six fields (with ten positions their tuples still have 64-bit ids), twelve positions
    for action in (ok, dict(ok, positions=[29903, 1]), dict(ok, positions=list(range(1001, 1011)), groupByFields=fields, excludeIncomplete=True),
                   dict(ok, positions=list(range(1001, 1013)), groupByFields=fields[:1] + fields[2:4]),
                   dict(ok, sequenceName="testSecondSequence"), dict(ok, groupByFields=["country"], orderByFields=["country", "proportion", "count", "haplotype"]),
                   {"type": "AminoAcidHaplotypes", "sequenceName": "S", "positions": [1274, 501]}):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and document["queryResult"], (action, document)
        assert all(len(row["haplotype"]) == len(action["positions"]) for row in document["queryResult"])
        assert action.get("excludeIncomplete") or sum(row["count"] for row in document["queryResult"]) == 51


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        for action in ({"type": "Haplotypes", "positions": [1]}, {"type": "AminoAcidHaplotypes", "sequenceName": "S", "positions": [1]}):
            status, document = engine.execute_raw({"action": action, "filterExpression": TRUE})
            assert status == 400 and "sharded" in document["message"] and action["type"] in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
K5 = [40, 3, 17, 29, 8]                                  # 16^5 = 2^20 tuples: the dense histogram, at its limit
K6 = K5 + [22]                                           # 2^24: the hash table
K12 = K6 + [0, 47, 11, 35, 5, 26]                        # two id columns
STRETCH = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}


@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2027)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


@pytest.fixture(scope="module")
def synthetic_reference(synthetic):
    """(positions, filter, grouped) -> the reference's rows: computed once, whatever layout the store has."""
    sym, _, bucket = synthetic
    rows = np.arange(N_ROWS)
    in_range = (rows >= 30_000) & (rows <= 61_000)
    groups = [(int(b),) for b in bucket]
    want = {}
    for name, positions in (("k5", K5), ("k6", K6), ("k12", K12)):
        for expression, mask in ((TRUE, None), (STRETCH, in_range)):
            for grouped in (False, True):
                want[name, expression["type"], grouped] = _want(haplotype_rows(sym, positions, NUC_CHARS, mask=mask, groups=groups if grouped else None))
    # the second id column matters: positions 7 .. 12 split tuples that agree at the first six
    assert len(want["k12", "True", False]) > len(want["k6", "True", False]) > len(want["k5", "True", False]) > 3
    assert max(K12) < POSITIONS and len(set(K12)) == 12
    return want


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, synthetic_reference, layout, missing_runs):
    """140 003 rows x 48 positions: the symbol columns over derived symbols, runs of N, sparse ambiguity keys and code planes, then
    the dense histogram (k = 5), the hash table (k = 6) and two id columns (k = 12), for the whole store and a range of rows, with
    and without a metadata column in front."""
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        for name, positions in (("k5", K5), ("k6", K6), ("k12", K12)):
            for expression in (TRUE, STRETCH):
                for grouped in (False, True):
                    action = {"type": "Haplotypes", "positions": [p + 1 for p in positions], "groupByFields": ["bucket"] if grouped else []}
                    got = engine.execute_query({"action": action, "filterExpression": expression})
                    assert _as_dict(got, ("bucket",) if grouped else ()) == synthetic_reference[name, expression["type"], grouped], (layout, missing_runs, name, expression, grouped)
    finally:
        engine.close()
