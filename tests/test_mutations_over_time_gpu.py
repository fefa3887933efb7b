"""MutationsOverTime / AminoAcidMutationsOverTime: count and coverage per (mutation, date range) from the grouped count kernel
(K7), against counts taken from the raw aligned sequences, against Mutations under And(filter, DateBetween), and on synthetic
stores in every adaptive layout."""
import datetime
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402

NUC_VALID = "-ACGT"
AA_VALID = "-ACDEFGHIKLMNPQRSTVWY*"
NUC_CHARS = "-ACGTRYSWKMBDHVN"


def _build_example_engine(data, partition_sizes):
    from tests.test_engine_gpu import build_engine

    return build_engine(data, partition_sizes)


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, [37, 1, 62]], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data
    engine.close()


def _canonical(char):
    return {".": "-", "U": "T"}.get(char, char)


def _pick_mutations(data, is_aa, names, per_store=4):
    """Per store the positions with the most variation: the commonest non-reference symbol there and the reference symbol."""
    valid = AA_VALID if is_aa else NUC_VALID
    references = data["aa_references"] if is_aa else data["nuc_references"]
    picked = []
    for name in names:
        sequences = [s for s in (data["aa"] if is_aa else data["nuc"])[name] if s is not None]
        reference = references[name]
        scored = []
        for p in range(len(reference)):
            column = [_canonical(s[p]) for s in sequences if p < len(s)]
            others = {}
            for c in column:
                if c in valid and c != reference[p]:
                    others[c] = others.get(c, 0) + 1
            if others:
                symbol = max(sorted(others), key=lambda c: others[c])
                scored.append((others[symbol], p, symbol))
        for _, p, symbol in sorted(scored, reverse=True)[:per_store]:
            picked.append(f"{name}:{reference[p]}{p + 1}{symbol}")
            if reference[p] in valid:
                picked.append(f"{name}:{p + 1}{reference[p]}")
    return picked


def _parse(mutation, default):
    name, _, rest = mutation.rpartition(":")
    name = name or default
    digits = "".join(c for c in rest if c.isdigit())
    return name, int(digits) - 1, rest[-1]


def _expected(oracle_db, data, query_action, filter_expression, is_aa):
    """The table from the raw aligned sequences of the rows the oracle selects for the filter."""
    keys = {row["gisaid_epi_isl"] for row in so.execute_query(
        oracle_db, {"action": {"type": "Details", "fields": ["gisaid_epi_isl"]}, "filterExpression": filter_expression})}
    valid = AA_VALID if is_aa else NUC_VALID
    references = data["aa_references"] if is_aa else data["nuc_references"]
    sequences = data["aa"] if is_aa else data["nuc"]
    field = query_action["dateField"]
    out = []
    for mutation in query_action["mutations"]:
        name, p, symbol = _parse(mutation, "main")
        for date_range in query_action["dateRanges"]:
            low = so.string_to_date(date_range["dateFrom"]) if date_range.get("dateFrom") else 1
            high = so.string_to_date(date_range["dateTo"]) if date_range.get("dateTo") else 0xFFFFFFFF
            count = coverage = 0
            for i, row in enumerate(data["rows"]):
                date = so.string_to_date(row.get(field) or "")
                if row["gisaid_epi_isl"] not in keys or date == 0 or not (low <= date <= high):
                    continue
                sequence = sequences[name][i]
                char = _canonical(sequence[p]) if sequence is not None else "X"
                if char in valid:
                    coverage += 1
                    count += char == symbol
            out.append({"count": count, "coverage": coverage, "dateFrom": date_range.get("dateFrom"), "dateTo": date_range.get("dateTo"),
                        "mutation": f"{references[name][p]}{p + 1}{symbol}", "sequenceName": name})
    return out


EXAMPLE_RANGES = [
    {"dateFrom": None, "dateTo": "2020-12-31"},
    {"dateFrom": "2021-01-01", "dateTo": "2021-01-31"},
    {"dateFrom": "2021-02-01", "dateTo": "2021-03-31"},
    {"dateFrom": "2021-04-01", "dateTo": "2021-04-03"},  # no rows
    {"dateFrom": "2021-05-01", "dateTo": None},
]
EXAMPLE_FILTERS = [
    {"type": "True"},
    {"type": "PangoLineage", "column": "pango_lineage", "value": "B.1.1.7", "includeSublineages": True},
    {"type": "Not", "child": {"type": "PangoLineage", "column": "pango_lineage", "value": "B.1.1.7", "includeSublineages": True}},
]


def test_example_dataset_matches_raw_sequences(example):
    engine, oracle_db, data = example
    nuc = _pick_mutations(data, False, ["main", "testSecondSequence"])
    nuc.append(nuc[0].split(":", 1)[1])  # the default nucleotide sequence, no name
    aa = _pick_mutations(data, True, ["S", "N", "ORF1a"], per_store=3)
    assert len(nuc) > 6 and len(aa) > 6
    for filter_expression in EXAMPLE_FILTERS:
        for action_type, mutations, is_aa in (("MutationsOverTime", nuc, False), ("AminoAcidMutationsOverTime", aa, True)):
            for field in ("date", "unsorted_date"):
                action = {"type": action_type, "mutations": mutations, "dateField": field, "dateRanges": EXAMPLE_RANGES}
                got = engine.execute_query({"action": action, "filterExpression": filter_expression})
                want = _expected(oracle_db, data, action, filter_expression, is_aa)
                assert got == want, json.dumps(action)
    # the dense matrix really has rows with count 0 and coverage 0 as well as non-zero ones
    assert any(row["coverage"] == 0 for row in got) and any(row["count"] > 0 for row in got)


def test_example_dataset_agrees_with_mutations_action(example):
    engine, _, data = example
    mutations = _pick_mutations(data, False, ["main"], per_store=6)
    ranges = EXAMPLE_RANGES
    for filter_expression in EXAMPLE_FILTERS:
        got = engine.execute_query({"action": {"type": "MutationsOverTime", "mutations": mutations, "dateField": "date", "dateRanges": ranges},
                                    "filterExpression": filter_expression})
        for k, date_range in enumerate(ranges):
            scan = engine.execute_query({"action": {"type": "Mutations", "minProportion": 0, "sequenceName": "main"},
                                         "filterExpression": {"type": "And", "children": [
                                             filter_expression,
                                             {"type": "DateBetween", "column": "date", "from": date_range["dateFrom"], "to": date_range["dateTo"]}]}})
            by_name = {row["mutation"]: row for row in scan}
            rows = got[k::len(ranges)]
            for row in rows:
                assert (row["dateFrom"], row["dateTo"]) == (date_range["dateFrom"], date_range["dateTo"])
                if row["count"] > 0 and row["mutation"][0] != row["mutation"][-1]:
                    other = by_name[row["mutation"]]
                    assert other["count"] == row["count"]
                    assert other["proportion"] == row["count"] / row["coverage"]
                elif row["mutation"][0] != row["mutation"][-1]:
                    assert row["mutation"] not in by_name


def test_order_limit_offset(example):
    engine, _, data = example
    mutations = _pick_mutations(data, False, ["main"], per_store=3)
    base = {"type": "MutationsOverTime", "mutations": mutations, "dateField": "date", "dateRanges": EXAMPLE_RANGES}
    rows = engine.execute_query({"action": base, "filterExpression": {"type": "True"}})
    assert len(rows) == len(mutations) * len(EXAMPLE_RANGES)
    ordered = engine.execute_query({"action": dict(base, orderByFields=[{"field": "coverage", "order": "descending"}, "mutation", "dateFrom"],
                                                   limit=4, offset=1), "filterExpression": {"type": "True"}})
    assert len(ordered) == 4
    assert [r["coverage"] for r in ordered] == sorted([r["coverage"] for r in ordered], reverse=True)
    status, document = engine.execute_raw({"action": dict(base, orderByFields=["proportion"]), "filterExpression": {"type": "True"}})
    assert status == 400, document


def _error_cases(data):
    reference = data["nuc_references"]["main"]
    wrong = next(c for c in "ACGT" if c != reference[99])
    ranges = [{"dateFrom": "2021-01-01", "dateTo": "2021-01-31"}]
    ok = {"type": "MutationsOverTime", "mutations": ["100A"], "dateField": "date", "dateRanges": ranges}
    cases = [
        {k: v for k, v in ok.items() if k != "mutations"},
        dict(ok, mutations="100A"),
        dict(ok, mutations=[100]),
        {k: v for k, v in ok.items() if k != "dateField"},
        dict(ok, dateField=3),
        {k: v for k, v in ok.items() if k != "dateRanges"},
        dict(ok, dateRanges={"dateFrom": None}),
        dict(ok, dateRanges=["2021-01-01"]),
        dict(ok, mutations=["nosuchsequence:100A"]),
        dict(ok, type="AminoAcidMutationsOverTime", mutations=["D614G"]),
        dict(ok, type="AminoAcidMutationsOverTime", mutations=["nosuchgene:D614G"]),
        dict(ok, mutations=["0A"]),
        dict(ok, mutations=[f"{len(reference) + 1}A"]),
        dict(ok, mutations=["100N"]),
        dict(ok, mutations=["100"]),
        dict(ok, mutations=["A"]),
        dict(ok, type="AminoAcidMutationsOverTime", mutations=["S:10J"]),
        dict(ok, mutations=[f"{wrong}100A"]),
        dict(ok, dateField="region"),
        dict(ok, dateField="age"),
        dict(ok, dateField="nosuchcolumn"),
        dict(ok, dateRanges=[{"dateFrom": "2021-13-45", "dateTo": None}]),
        dict(ok, dateRanges=[{"dateFrom": "yesterday", "dateTo": None}]),
        dict(ok, dateRanges=[{"dateFrom": 20210101, "dateTo": None}]),
        dict(ok, dateRanges=[{"dateFrom": "2021-02-01", "dateTo": "2021-01-01"}]),
        dict(ok, dateRanges=[{"dateFrom": "2021-01-01", "dateTo": "2021-01-31"}, {"dateFrom": "2021-01-31", "dateTo": "2021-02-28"}]),
        dict(ok, dateRanges=[{"dateFrom": None, "dateTo": "2021-01-31"}, {"dateFrom": "2020-06-01", "dateTo": None}]),
        dict(ok, dateRanges=[{"dateFrom": f"2021-01-{1 + k % 28:02d}", "dateTo": f"2021-01-{1 + k % 28:02d}"} for k in range(1025)]),
        dict(ok, mutations=["100A"] * 4097),
    ]
    return cases


def test_each_validation_error_is_a_bad_request(example):
    engine, _, data = example
    for action in _error_cases(data):
        status, document = engine.execute_raw({"action": action, "filterExpression": {"type": "True"}})
        assert status == 400, (json.dumps(action)[:200], document)
        assert document["error"] == "Bad request"
    # the limits themselves are accepted
    day = datetime.date(2020, 1, 1)
    ranges = [{"dateFrom": str(day + datetime.timedelta(k)), "dateTo": str(day + datetime.timedelta(k))} for k in range(1024)]
    status, document = engine.execute_raw({"action": {"type": "MutationsOverTime", "mutations": ["100A", "main:100C"], "dateField": "date",
                                                      "dateRanges": ranges}, "filterExpression": {"type": "True"}})
    assert status == 200 and len(document["queryResult"]) == 2048, document
    status, document = engine.execute_raw({"action": {"type": "MutationsOverTime", "mutations": ["100A"] * 4096, "dateField": "date",
                                                      "dateRanges": ranges[:2]}, "filterExpression": {"type": "True"}})
    assert status == 200 and len(document["queryResult"]) == 8192


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        status, document = engine.execute_raw({"action": {"type": "MutationsOverTime", "mutations": ["100A"], "dateField": "date",
                                                          "dateRanges": [{"dateFrom": None, "dateTo": None}]}, "filterExpression": {"type": "True"}})
        assert status == 400 and "sharded" in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout ------------------------------------------------------------------------------
N_ROWS = 140_003
POSITIONS = 48
EPOCH = datetime.date(2021, 1, 1)


def _synthetic_matrix(rng):
    from tests.test_kernels_gpu import settle_positions, skewed_symbols

    sym = skewed_symbols(rng, N_ROWS, POSITIONS, "nuc")
    settle_positions(rng, sym, range(0, POSITIONS, 2), "nuc")
    sym[:, 5] = rng.integers(0, 16, size=N_ROWS)  # many frequent symbols: code planes / identity
    # runs of N: amplicon drop-outs and unsequenced ends
    for row in rng.choice(N_ROWS, size=N_ROWS // 20, replace=False):
        start = int(rng.integers(0, POSITIONS))
        sym[row, start:start + int(rng.integers(1, 12))] = 15
    sym[rng.choice(N_ROWS, size=300, replace=False), :] = 15  # whole genomes missing
    # ambiguity codes
    cells = rng.integers(0, N_ROWS * POSITIONS, size=N_ROWS // 10)
    sym.reshape(-1)[cells] = rng.integers(5, 15, size=len(cells))
    return sym


def _synthetic_dates(rng):
    """Days since EPOCH, mostly in (block, date) order like a sorted store, some scattered, some NULL (-1)."""
    blocks = np.concatenate([np.sort(rng.integers(0, 200, size=size)) for size in np.diff(np.linspace(0, N_ROWS, 60).astype(int))])
    scattered = rng.choice(N_ROWS, size=N_ROWS // 50, replace=False)
    blocks[scattered] = rng.integers(0, 200, size=len(scattered))
    blocks[rng.choice(N_ROWS, size=500, replace=False)] = -1
    return blocks


def _day(k):
    return str(EPOCH + datetime.timedelta(int(k)))


SYNTHETIC_RANGES = [(7 * w, 7 * w + 6) for w in range(10)] + [(150, None), (None, -1)]  # the last: no rows


def _range_json(low, high):
    return {"dateFrom": None if low is None else _day(low), "dateTo": None if high is None else _day(high)}


@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2024)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


def _synthetic_engine(sym, days, bucket):
    from silo_amd.engine import Engine

    reference = "".join(NUC_VALID[1 + (p % 4)] for p in range(POSITIONS))
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": reference}], "genes": []})
    engine.set_schema("key", "date")
    part = engine.add_partition(N_ROWS)
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    engine.append_sequences(part, "main", False, 0, [bytes(row).decode() for row in lut[sym]])
    engine.append_metadata(part, "key", "string", [str(i) for i in range(N_ROWS)])
    engine.append_metadata(part, "date", "date", ["" if d < 0 else _day(d) for d in days])
    engine.append_metadata(part, "row", "int", [str(i) for i in range(N_ROWS)])
    engine.append_metadata(part, "bucket", "int", [str(b) for b in bucket])
    engine.finalize()
    return engine, reference


SYNTHETIC_FILTERS = [
    ({"type": "True"}, lambda rows, bucket: np.ones(len(rows), dtype=bool)),
    ({"type": "IntEquals", "column": "bucket", "value": 7}, lambda rows, bucket: bucket == 7),
    ({"type": "IntBetween", "column": "row", "from": 30_000, "to": 61_000}, lambda rows, bucket: (rows >= 30_000) & (rows <= 61_000)),
]


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_numpy(built, synthetic, layout, missing_runs):
    from silo_amd import binding

    sym, days, bucket = synthetic
    lib = binding.load_library()
    lib.silo_gpu_tune(4, layout)
    lib.silo_gpu_tune(9, -1)
    lib.silo_gpu_tune(8, missing_runs)
    try:
        engine, reference = _synthetic_engine(sym, days, bucket)
    finally:
        lib.silo_gpu_tune(4, 0)
        lib.silo_gpu_tune(9, 0)
        lib.silo_gpu_tune(8, 0)
    try:
        # every position: the most numerous valid symbol (derived where the layout derives one) and two others
        mutations = []
        for p in range(POSITIONS):
            column = sym[:, p]
            counts = np.bincount(column[column <= 4], minlength=5)
            for s in np.argsort(-counts, kind="stable")[:2].tolist() + [int(np.argmin(counts))]:
                mutations.append((p, s))
        texts = [f"{p + 1}{NUC_VALID[s]}" if k % 2 else f"main:{reference[p]}{p + 1}{NUC_VALID[s]}" for k, (p, s) in enumerate(mutations)]
        rows = np.arange(N_ROWS)
        valid = sym <= 4
        for expression, select in SYNTHETIC_FILTERS:
            selected = select(rows, bucket)
            action = {"type": "MutationsOverTime", "mutations": texts, "dateField": "date",
                      "dateRanges": [_range_json(low, high) for low, high in SYNTHETIC_RANGES]}
            got = engine.execute_query({"action": action, "filterExpression": expression})
            assert len(got) == len(mutations) * len(SYNTHETIC_RANGES)
            k = 0
            for p, s in mutations:
                for low, high in SYNTHETIC_RANGES:
                    in_range = selected & (days >= (0 if low is None else low)) & (days <= (10 ** 6 if high is None else high))
                    want_count = int(np.count_nonzero(in_range & (sym[:, p] == s)))
                    want_coverage = int(np.count_nonzero(in_range & valid[:, p]))
                    row = got[k]
                    k += 1
                    assert row["mutation"] == f"{reference[p]}{p + 1}{NUC_VALID[s]}"
                    assert (row["count"], row["coverage"]) == (want_count, want_coverage), (layout, missing_runs, expression, p, s, low, high)
            assert any(r["count"] > 0 for r in got) and any(r["coverage"] == 0 for r in got)
    finally:
        engine.close()
