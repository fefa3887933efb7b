"""NearestAmong: for every sequence the filter selects (a subject) its `neighbours` closest sequences among those `among` selects (the
candidates) — another database row, "distance <= maxDistance and comparedPositions >= minComparedPositions", lowest by (distance,
candidate number) — from the rectangle kernel and the per-row selection (K14), through JSON and the engine: against the numpy
reference of tests/neighbours_reference.py on the strings the oracle's FastaAligned returns for both filters, against the engine's own
NearestNeighbours and DistanceMatrix, and on synthetic stores in every adaptive layout against the reference on the raw symbol matrix.
The lists are unique, so every comparison is an exact equality."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402
from tests import dataset  # noqa: E402
from tests.neighbours_reference import NOT_ELIGIBLE, cells_of, cross_counts, nearest_columns  # noqa: E402
from tests.pair_distances_reference import AA_VALID, NUC_CHARS, NUC_VALID  # noqa: E402
from tests.test_distance_matrix_gpu import PARTITION_SIZES, _key_is, _tuned_engine  # noqa: E402
from tests.test_mutations_over_time_gpu import N_ROWS, _build_example_engine, _synthetic_dates, _synthetic_matrix  # noqa: E402
from tests.test_oracle_golden import build_oracle_db  # noqa: E402
from tests.test_queries_over_time_gpu import LINEAGE  # noqa: E402

FIELDS = {"key", "neighbourKey", "rank", "distance", "comparedPositions"}
K = 3
# (sequenceName, its valid symbols, a maxDistance under which some sequences of the example data have fewer than K neighbours): the
# default nucleotide sequence and a gene — gene S has 24 sequences within 1 of each other, so K = 3 ties
SEQUENCES = [(None, NUC_VALID, 16), ("S", AA_VALID, 1)]
TRUE = {"type": "True"}
FALSE = {"type": "False"}


@pytest.fixture(scope="module")
def example_data():
    return dataset.load_example_dataset()


@pytest.fixture(scope="module", params=[None, PARTITION_SIZES], ids=["1-partition", "3-partitions"])
def example(request, built, example_data):
    engine = _build_example_engine(example_data, request.param)
    oracle_db = build_oracle_db(example_data, request.param)
    yield engine, oracle_db, example_data, request.param
    engine.close()


_CHARS = {}   # (sequence, filter) -> (keys, chars): the oracle's FastaAligned takes seconds per call, so each is asked once — its
#               answer does not depend on how the rows are cut into partitions — and shared, unchanged, by the tests
_COUNTS = {}  # (sequence, subjects' filter, candidates' filter) -> (self columns, differing, compared)


def _chars(oracle_db, sequence_name, expression):
    name = sequence_name or "main"
    cached = (name, json.dumps(expression, sort_keys=True))
    if cached not in _CHARS:
        selected = so.execute_query(oracle_db, {"action": {"type": "FastaAligned", "sequenceName": name}, "filterExpression": expression})
        chars = np.array([list(row[name].encode()) for row in selected], dtype=np.uint8).reshape(len(selected), -1) if selected else np.zeros((0, 0), np.uint8)
        _CHARS[cached] = ([row["gisaid_epi_isl"] for row in selected], chars)
    return _CHARS[cached]


def _counts(oracle_db, sequence_name, valid_chars, subjects, among):
    """(the subjects' keys, the candidates' keys, self columns, differing, compared) for the two filters."""
    subject_keys, subject_chars = _chars(oracle_db, sequence_name, subjects)
    candidate_keys, candidate_chars = _chars(oracle_db, sequence_name, among)
    cached = (sequence_name, json.dumps(subjects, sort_keys=True), json.dumps(among, sort_keys=True))
    if cached not in _COUNTS:
        number = {key: column for column, key in enumerate(candidate_keys)}
        self_columns = np.array([number.get(key, NOT_ELIGIBLE) for key in subject_keys], dtype=np.uint32)
        if len(subject_keys) == 0 or len(candidate_keys) == 0:
            counts = (np.zeros((len(subject_keys), len(candidate_keys)), np.uint32),) * 2
        else:
            counts = cross_counts(subject_chars, candidate_chars, valid_chars)
        _COUNTS[cached] = (self_columns, *counts)
    return (subject_keys, candidate_keys, *_COUNTS[cached])


def _rows_of(subject_keys, candidate_keys, self_columns, differing, compared, k, max_distance=NOT_ELIGIBLE, min_compared=0):
    """(the rows of the response, the cells, the lists, the counts) of the reference."""
    if len(subject_keys) == 0 or len(candidate_keys) == 0:
        return [], np.zeros((len(subject_keys), len(candidate_keys), 2), np.uint32), np.zeros((len(subject_keys), k, 3), np.uint32), np.zeros(len(subject_keys), np.uint32)
    cells = cells_of(differing, compared, self_columns, max_distance, min_compared)
    lists, counts = nearest_columns(cells, k)
    rows = [
        {"key": subject_keys[s], "neighbourKey": candidate_keys[int(column)], "rank": r + 1, "distance": int(distance), "comparedPositions": int(positions)}
        for s in range(len(subject_keys))
        for r, (column, distance, positions) in enumerate(lists[s, :counts[s]])
    ]
    return rows, cells, lists, counts


def _action(sequence_name, among=None, **fields):
    action = dict(fields, type="NearestAmong")
    if sequence_name is not None:
        action["sequenceName"] = sequence_name
    if among is not None:
        action["among"] = among
    return action


def _ties_across_the_kth_place(cells, lists, counts, k):
    """Subjects whose k-th listed distance is also the distance of an eligible candidate that is not listed."""
    return sum(1 for s in range(len(counts)) if counts[s] == k and (cells[s, :, 0] == lists[s, k - 1, 1]).sum() > (lists[s, :k, 1] == lists[s, k - 1, 1]).sum())


def _filters(oracle_db, data):
    """(the subjects' filters, the candidates' filters): all rows, a lineage, keys spanning partitions, one row, no row; and all
    rows, the lineage and the keys again (the same filter), keys outside the lineage (disjoint from it), keys that overlap the
    first keys in part, no row."""
    lineage_keys = set(_chars(oracle_db, "S", LINEAGE)[0])
    outside = [row for row, key in enumerate(data["keys"]) if key not in lineage_keys]
    spanning = _key_is(data, 40, 3, 99, 57, 38)   # rows of the third partition and one of the first
    one = _key_is(data, 37)                       # the only row of the second partition
    overlapping = _key_is(data, 40, 3, 12, 60, 37)
    disjoint = _key_is(data, *(outside[:3] + outside[-3:]))
    assert 0 < len(lineage_keys) < 100 and len(outside) >= 6
    return [TRUE, LINEAGE, spanning, one, FALSE], [TRUE, LINEAGE, spanning, disjoint, overlapping, FALSE]


def test_example_dataset_matches_the_reference_on_the_oracles_sequences(example):
    engine, oracle_db, data, partition_sizes = example
    subject_filters, candidate_filters = _filters(oracle_db, data)
    partition_of = {key: int(np.searchsorted(np.cumsum(PARTITION_SIZES), row, side="right")) for row, key in enumerate(data["keys"])}
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        for subjects in subject_filters:
            for among in candidate_filters:
                counts = _counts(oracle_db, sequence_name, valid_chars, subjects, among)
                for bound in (None, max_distance):
                    want, cells, lists, listed = _rows_of(*counts, K, NOT_ELIGIBLE if bound is None else bound)
                    if subjects == TRUE and among == TRUE:  # the reference itself: a tie across the K-th place; under the bound, fewer than K
                        if bound is None:
                            assert _ties_across_the_kth_place(cells, lists, listed, K) > 0 and (listed == K).all(), sequence_name
                        else:
                            assert 0 < (listed < K).sum() < len(listed) and (listed == 0).any() and (listed == K).any(), sequence_name
                    if subjects == LINEAGE and among == candidate_filters[3]:
                        assert (counts[2] == NOT_ELIGIBLE).all()  # really disjoint: no subject is a candidate
                    if subjects == subject_filters[2] and among == candidate_filters[4]:
                        assert 0 < (counts[2] != NOT_ELIGIBLE).sum() < len(counts[0])  # really overlapping in part
                    fields = {} if bound is None else {"maxDistance": bound}
                    got = engine.execute_query({"action": _action(sequence_name, among, neighbours=K, **fields), "filterExpression": subjects})
                    assert got == want, (sequence_name, subjects, among, bound)
                    assert all(set(row) == FIELDS for row in got)
                    if FALSE in (subjects, among):
                        assert got == []
        if partition_sizes is not None:  # a neighbour that lies in another partition than its subject
            everything = engine.execute_query({"action": _action(sequence_name, TRUE, neighbours=K), "filterExpression": TRUE})
            assert any(partition_of[row["key"]] != partition_of[row["neighbourKey"]] for row in everything)


def test_among_absent_is_the_querys_own_filter_and_one_neighbour_is_the_default(example):
    engine, oracle_db, data, _ = example
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        for expression in (TRUE, LINEAGE, _key_is(data, 40, 3, 99, 57, 38), _key_is(data, 37)):
            for fields in ({"neighbours": K}, {"neighbours": K, "maxDistance": max_distance}, {}):
                absent = engine.execute_query({"action": _action(sequence_name, None, **fields), "filterExpression": expression})
                given = engine.execute_query({"action": _action(sequence_name, expression, **fields), "filterExpression": expression})
                assert absent == given
                want = _rows_of(*_counts(oracle_db, sequence_name, valid_chars, expression, expression), fields.get("neighbours", 1), fields.get("maxDistance", NOT_ELIGIBLE))[0]
                assert absent == want and all(row["key"] != row["neighbourKey"] for row in absent)
            if expression == _key_is(data, 37):
                assert absent == []  # one sequence, which is not its own neighbour


def test_min_compared_positions_from_the_references_counts(example):
    engine, oracle_db, _, _ = example
    for sequence_name, valid_chars, max_distance in SEQUENCES:
        counts = _counts(oracle_db, sequence_name, valid_chars, LINEAGE, TRUE)
        unbounded, _, lists, listed = _rows_of(*counts, K)
        positions = np.sort(lists[..., 2][np.arange(K)[None, :] < listed[:, None]])
        c = int(positions[len(positions) // 2])  # a count that occurs among the listed neighbours
        seen = set()
        for bound, min_compared in ((None, c), (None, c + 1), (max_distance, c), (None, 2**31 - 1)):
            want = _rows_of(*counts, K, NOT_ELIGIBLE if bound is None else bound, min_compared)[0]
            fields = {"minComparedPositions": min_compared, **({} if bound is None else {"maxDistance": bound})}
            got = engine.execute_query({"action": _action(sequence_name, TRUE, neighbours=K, **fields), "filterExpression": LINEAGE})
            assert got == want, (sequence_name, bound, min_compared)
            assert all(row["comparedPositions"] >= min_compared for row in got)
            seen.add(json.dumps(got))
        assert len(seen) == 4 and json.dumps(unbounded) not in seen and "[]" in seen  # every bound changes the answer; the last leaves nothing


def test_every_subjects_rows_are_its_nearest_neighbours_and_its_best_distance_matrix_rows(example):
    engine, oracle_db, data, _ = example
    spanning, overlapping = _key_is(data, 40, 3, 99, 57, 38), _key_is(data, 40, 3, 12, 60, 37)
    for sequence_name, _, max_distance in SEQUENCES:
        named = {} if sequence_name is None else {"sequenceName": sequence_name}
        for subjects, among in ((LINEAGE, TRUE), (spanning, overlapping), (overlapping, LINEAGE)):
            subject_keys = _chars(oracle_db, sequence_name, subjects)[0]
            number = {key: column for column, key in enumerate(_chars(oracle_db, sequence_name, among)[0])}
            union = {"type": "Or", "children": [subjects, among]}
            matrix = engine.execute_query({"action": dict(named, type="DistanceMatrix"), "filterExpression": union})
            for fields in ({}, {"maxDistance": max_distance}):
                got = engine.execute_query({"action": _action(sequence_name, among, neighbours=K, **fields), "filterExpression": subjects})
                assert len(got) > 0
                for key in subject_keys:
                    mine = [row for row in got if row["key"] == key]
                    assert [row["rank"] for row in mine] == list(range(1, len(mine) + 1))
                    listed = [{"primaryKey": row["neighbourKey"], "distance": row["distance"], "comparedPositions": row["comparedPositions"]} for row in mine]
                    nearest = engine.execute_query({"action": dict(named, type="NearestNeighbours", primaryKey=key, neighbours=K, **fields), "filterExpression": among})
                    assert nearest == listed, (sequence_name, key, fields)
                    pairs = [(row["distance"], number[other], other, row["comparedPositions"]) for row in matrix
                             for other in ([row["secondKey"]] if row["firstKey"] == key else [row["firstKey"]] if row["secondKey"] == key else [])
                             if other in number and row["distance"] <= fields.get("maxDistance", 2**31)]
                    best = [{"primaryKey": other, "distance": distance, "comparedPositions": positions} for distance, _, other, positions in sorted(pairs)[:K]]
                    assert best == listed, (sequence_name, key, fields)


def test_order_limit_offset(example):
    engine, _, _, _ = example
    for sequence_name, _, _ in SEQUENCES:
        base = _action(sequence_name, TRUE, neighbours=K)
        got = engine.execute_query({"action": base, "filterExpression": LINEAGE})
        assert [row["rank"] for row in got[:2 * K]] == list(range(1, K + 1)) * 2  # by subject, then rank
        assert len({row["distance"] for row in got}) >= 3
        orders = [
            (["key", "rank"], lambda row: (row["key"], row["rank"])),
            (["neighbourKey", "key"], lambda row: (row["neighbourKey"], row["key"])),
            ([{"field": "rank", "order": "descending"}, "key"], lambda row: (-row["rank"], row["key"])),
            ([{"field": "distance", "order": "descending"}, "neighbourKey", "key"], lambda row: (-row["distance"], row["neighbourKey"], row["key"])),
            (["comparedPositions", "key", "rank"], lambda row: (row["comparedPositions"], row["key"], row["rank"])),
        ]
        for order_by, in_python in orders:
            want = sorted(got, key=in_python)
            assert want != got
            for limit, offset in ((7, 3), (100_000, 0), (5, len(got) - 2)):
                ordered = engine.execute_query({"action": dict(base, orderByFields=order_by, limit=limit, offset=offset), "filterExpression": LINEAGE})
                assert ordered == want[offset:offset + limit], order_by
        assert engine.execute_query({"action": dict(base, limit=4, offset=2), "filterExpression": LINEAGE}) == got[2:6]


def test_each_validation_error_is_a_bad_request_that_names_the_field(example):
    engine, _, _, _ = example
    ok = {"type": "NearestAmong"}
    cases = [
        (dict(ok, neighbours=0), "neighbours"),
        (dict(ok, neighbours=65), "neighbours"),
        (dict(ok, neighbours=-1), "neighbours"),
        (dict(ok, neighbours=1.5), "neighbours"),
        (dict(ok, neighbours="3"), "neighbours"),
        (dict(ok, neighbours=None), "neighbours"),
        (dict(ok, maxDistance=-1), "maxDistance"),
        (dict(ok, maxDistance=1.5), "maxDistance"),
        (dict(ok, maxDistance="2"), "maxDistance"),
        (dict(ok, maxDistance=None), "maxDistance"),
        (dict(ok, maxDistance=2**31), "maxDistance"),
        (dict(ok, minComparedPositions=-1), "minComparedPositions"),
        (dict(ok, minComparedPositions=0.5), "minComparedPositions"),
        (dict(ok, minComparedPositions="1"), "minComparedPositions"),
        (dict(ok, minComparedPositions=None), "minComparedPositions"),
        (dict(ok, minComparedPositions=2**31), "minComparedPositions"),
        (dict(ok, among=5), "among"),
        (dict(ok, among="True"), "among"),
        (dict(ok, among=None), "among"),
        (dict(ok, among=[TRUE]), "among"),
        (dict(ok, among={"type": "NoSuchFilter"}), "among"),
        (dict(ok, among={"column": "pango_lineage"}), "among"),
        (dict(ok, among={"type": "FloatBetween", "column": "nosuchcolumn", "from": 0.5, "to": 1.5}), "nosuchcolumn"),
        (dict(ok, sequenceName=3), "sequenceName"),
        (dict(ok, sequenceName=["main"]), "sequenceName"),
        (dict(ok, sequenceName="nosuchsequence"), "Database does not contain a sequence with name: 'nosuchsequence'"),
        (dict(ok, orderByFields=["primaryKey"]), "primaryKey"),
        (dict(ok, orderByFields=[{"field": "gisaid_epi_isl", "order": "ascending"}]), "gisaid_epi_isl"),
    ]
    for action, named in cases:
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 400, (action, document)
        assert document["error"] == "Bad request" and named in document["message"], (named, document)
    for action in (ok, dict(ok, neighbours=64, maxDistance=0, minComparedPositions=0), dict(ok, maxDistance=2**31 - 1, minComparedPositions=1, among=TRUE),
                   dict(ok, sequenceName="testSecondSequence"),
                   dict(ok, sequenceName="ORF1a", orderByFields=["key", "neighbourKey", "rank", "distance", "comparedPositions"])):
        status, document = engine.execute_raw({"action": action, "filterExpression": LINEAGE})
        assert status == 200 and document["queryResult"] and all(set(row) == FIELDS for row in document["queryResult"]), document
    status, document = engine.execute_raw({"action": dict(ok, minComparedPositions=2**31 - 1), "filterExpression": LINEAGE})
    assert status == 200 and document["queryResult"] == []  # no pair compares at that many positions: nothing is eligible, no row


def test_sharded_engine_refuses(built, example_data):
    engine = _build_example_engine(example_data, None)
    try:
        engine.set_sharding(0, 2, False)
        status, document = engine.execute_raw({"action": {"type": "NearestAmong"}, "filterExpression": TRUE})
        assert status == 400 and "sharded" in document["message"] and "NearestAmong" in document["message"], document
    finally:
        engine.close()


# ---- synthetic stores in every adaptive layout --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2026)
    sym = _synthetic_matrix(rng)
    days = _synthetic_dates(rng)
    bucket = rng.integers(0, 1000, size=N_ROWS)
    return sym, days, bucket


_SYNTHETIC_COUNTS = {}


def _synthetic_expected(sym, subjects, candidates, label, k, max_distance, min_compared):
    """_rows_of for the rows that the two masks mark; the two counts per pair are computed once per pair of selections."""
    subject_rows, candidate_rows = np.flatnonzero(subjects), np.flatnonzero(candidates)
    if label not in _SYNTHETIC_COUNTS:
        lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
        column_of = np.full(N_ROWS, NOT_ELIGIBLE, dtype=np.uint32)
        column_of[candidate_rows] = np.arange(len(candidate_rows))
        _SYNTHETIC_COUNTS[label] = (column_of[subject_rows], *cross_counts(lut[sym[subject_rows]], lut[sym[candidate_rows]], NUC_VALID))
    return _rows_of([str(row) for row in subject_rows], [str(row) for row in candidate_rows], *_SYNTHETIC_COUNTS[label], k, max_distance, min_compared)


@pytest.mark.parametrize("layout,missing_runs", [(0, 0), (3, 0), (2, 0), (-1, 0), (0, -1)],
                         ids=["derived", "one-hot", "code-planes", "identity", "missing-plane"])
def test_adaptive_layouts_match_the_reference(built, synthetic, layout, missing_runs):
    """140 003 rows x 48 positions: the composition reconstruct -> pack (twice) -> cross -> nearest columns over derived symbols, runs
    of N, sparse ambiguity keys and code planes, for a scattered selection of about 140 rows against a stretch of 401, and that
    stretch against candidates that hold half of it."""
    sym, _, bucket = synthetic
    engine = _tuned_engine(synthetic, layout, missing_runs)
    try:
        rows = np.arange(N_ROWS)
        in_bucket = {"type": "IntEquals", "column": "bucket", "value": 7}
        stretch = {"type": "IntBetween", "column": "row", "from": 30_000, "to": 30_400}
        later = {"type": "Or", "children": [in_bucket, {"type": "IntBetween", "column": "row", "from": 30_200, "to": 30_600}]}
        in_stretch = (rows >= 30_000) & (rows <= 30_400)
        cases = (("bucket-stretch", in_bucket, bucket == 7, stretch, in_stretch),
                 ("stretch-later", stretch, in_stretch, later, (bucket == 7) | ((rows >= 30_200) & (rows <= 30_600))))
        for label, subjects, subject_mask, among, candidate_mask in cases:
            m = int(subject_mask.sum())
            for fields, bounds in (({}, (NOT_ELIGIBLE, 0)), ({"maxDistance": 0, "minComparedPositions": 46}, (0, 46))):
                want, cells, lists, listed = _synthetic_expected(sym, subject_mask, candidate_mask, label, 5, *bounds)
                if bounds == (NOT_ELIGIBLE, 0):
                    assert (listed == 5).all() and _ties_across_the_kth_place(cells, lists, listed, 5) > m // 2
                else:
                    assert m // 10 < (listed == 0).sum() < (listed < 5).sum() < m // 2  # some without a neighbour, some with fewer than 5
                got = engine.execute_query({"action": dict(fields, type="NearestAmong", among=among, neighbours=5), "filterExpression": subjects})
                assert got == want, (layout, missing_runs, label, bounds)
    finally:
        engine.close()


def test_the_limits_of_2048_subjects_and_8192_candidates(built, synthetic):
    """Subjects 0 .. 2047 against candidates 0 .. 8191 — one pack batch and four, cells of 128 MB, every column slot of a block —
    against the reference; subjects 0 .. 2048 and candidates 0 .. 8192: refused, each by its name."""
    sym, _, _ = synthetic
    engine = _tuned_engine(synthetic, 0, 0)
    try:
        def between(last):
            return {"type": "IntBetween", "column": "row", "from": 0, "to": last}

        rows = np.arange(N_ROWS)
        want, _, _, listed = _synthetic_expected(sym, rows < 2048, rows < 8192, "limit", K, 0, 46)
        assert 100 < (listed == 0).sum() < (listed < K).sum() < 500
        action = {"type": "NearestAmong", "neighbours": K, "maxDistance": 0, "minComparedPositions": 46}
        got = engine.execute_query({"action": dict(action, among=between(8191)), "filterExpression": between(2047)})
        assert got == want
        status, document = engine.execute_raw({"action": dict(action, among=between(8191)), "filterExpression": between(2048)})
        assert status == 400 and document["message"] == "NearestAmong action currently limited to 2048 subjects", document
        status, document = engine.execute_raw({"action": dict(action, among=between(8192)), "filterExpression": between(2047)})
        assert status == 400 and document["message"] == "NearestAmong action currently limited to 8192 candidates", document
    finally:
        engine.close()
