"""The end of a Mutations query: the finish kernel of a scan that selects the rows (k_finish_scan<true, 5 | 22>: the system-scope
fence only in the threads that stored a row, the block's ticket behind the barrier) and the response text written from the
delivered rows (host/mutation_rows_json.h), through the engine.

66 000 rows x 2 100 nucleotide positions — three finish blocks of 1 024 threads, the last partial — and a gene of 1 100 codons
(two blocks).  The rows come in four groups, chosen by an int column, so that the dense oracle alone decides where the selected
rows of a filter fall:
  group 0  ragged ends, runs of N, a frequent second symbol at the first and last positions of every block: rows in every block
  group 1  full-length rows, a second symbol in 30 % of them at three positions of the middle block: rows in that block only
  group 2  full-length rows, a second symbol at the first and the last position of every block
  group 3  the reference itself: no row at all
Every test asserts that placement on the oracle's rows before it looks at the engine's answer."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dense  # noqa: E402

TUNE_LAUNCH_COST, TUNE_FUSED_SELECT = 9, 13
N, POSITIONS, CODONS = 66_000, 2_100, 1_100
BLOCK = 1_024  # threads, so positions, of a finish block
NUC_CHARS = "-ACGTRYSWKMBDHVN"
AA_CHARS = "-ACDEFGHIKLMNPQRSTVWYBZ*X"
NUC_SCAN = list(range(5))                 # VALID_MUTATION_SYMBOLS as indexes into the characters: - A C G T
AA_SCAN = list(range(21)) + [23]          # - and the twenty amino acids, then the stop codon
GROUP_ROWS = (50_000, 6_000, 6_000, 4_000)
BLOCK_EDGES = (0, 1_023, 1_024, 2_047, 2_048, 2_099)
MIDDLE_ONLY = (1_100, 1_500, 2_000)
PROPORTION = 0.05


def alignment(rng, group, positions, letters, first_ambiguous, missing, frequent):
    """Symbol indexes [N][positions] and the reference: the reference's letter nearly everywhere, a second letter in 0.02 % of the
    rows of a position, other codes in 0.1 %; then per group what the module's docstring says.  frequent: {group: {position: share}}."""
    reference = rng.integers(1, letters + 1, size=positions).astype(np.uint8)
    second = ((reference % letters) + 1).astype(np.uint8)
    sym = np.empty((N, positions), dtype=np.uint8)
    for a in range(0, positions, 300):
        b = min(a + 300, positions)
        draw = rng.random((N, b - a), dtype=np.float32)
        share = np.full((N, b - a), 0.0002, dtype=np.float32)
        for g, places in frequent.items():
            for p, value in places.items():
                if a <= p < b:
                    share[group == g, p - a] = value
        chunk = np.where(draw < share, second[None, a:b], reference[None, a:b]).astype(np.uint8)
        lone = (draw >= share) & (draw < share + 0.001)
        chunk[lone] = rng.integers(first_ambiguous, missing + 1, size=int(lone.sum()))
        sym[:, a:b] = chunk
    ragged = np.flatnonzero(group == 0)
    end_mean = positions / 14
    lead = np.where(rng.random(len(ragged)) < 0.97, rng.geometric(1 / end_mean, size=len(ragged)), 0)
    trail = np.where(rng.random(len(ragged)) < 0.97, rng.geometric(1 / end_mean, size=len(ragged)), 0)
    column = np.arange(positions)
    for a in range(0, len(ragged), 8_192):
        rows = ragged[a:a + 8_192]
        part = sym[rows]
        part[column[None, :] < lead[a:a + 8_192, None]] = 0
        part[column[None, :] >= positions - trail[a:a + 8_192, None]] = 0
        sym[rows] = part
    for row in rng.choice(ragged, size=3_000, replace=False):  # runs of the missing symbol, some across the block borders
        start = int(rng.integers(0, positions))
        sym[row, start:start + int(rng.geometric(1 / end_mean))] = missing
    sym[group == 3] = reference[None, :]
    return sym, reference


def selected_rows(table, reference_index, proportion):
    """The row selection of a Mutations query over an exact table: (position, symbol, count, total), positions then symbols ascending."""
    covered = table.sum(axis=1, dtype=np.uint32)
    must_exceed = np.zeros(len(table), dtype=np.uint32)
    if proportion != 0:
        positive = covered > 0
        must_exceed[positive] = (np.ceil(covered[positive].astype(np.float64) * proportion) - 1).astype(np.uint32)
    passes = (table > must_exceed[:, None]) & (covered[:, None] > 0)
    passes[np.arange(len(table)), reference_index] = False
    return [(int(p), int(s), int(table[p, s]), int(covered[p])) for p, s in zip(*np.nonzero(passes))]


class Made:
    pass


@pytest.fixture(scope="module")
def made(built):
    from silo_amd import binding
    from silo_amd.engine import Engine

    rng = np.random.default_rng(211)
    group = np.repeat(np.arange(4), GROUP_ROWS)
    rng.shuffle(group)
    out = Made()
    out.lib = binding.load_library()
    out.group = group
    edges = {p: (0.08 if k % 2 == 0 else 0.6) for k, p in enumerate(BLOCK_EDGES)}
    out.nuc, out.nuc_reference = alignment(
        rng, group, POSITIONS, 4, 5, 15, {0: {**edges, 700: 0.08}, 1: {p: 0.3 for p in MIDDLE_ONLY}, 2: {p: 0.3 for p in BLOCK_EDGES}})
    out.aa, out.aa_reference = alignment(
        rng, group, CODONS, 20, 21, 24, {0: {0: 0.08, 500: 0.6, 1_023: 0.08, 1_024: 0.6, 1_099: 0.08}, 1: {1_030: 0.3, 1_090: 0.3}, 2: {0: 0.3, 1_023: 0.3, 1_024: 0.3}})
    stop = (group == 0) & (rng.random(N) < 0.08)
    out.aa[stop, 600] = 23  # the stop codon, the last of the valid symbols
    nuc_lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    aa_lut = np.frombuffer(AA_CHARS.encode(), dtype=np.uint8)
    out.lib.silo_gpu_tune(TUNE_LAUNCH_COST, -1)
    try:
        engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": bytes(nuc_lut[out.nuc_reference]).decode()}],
                         "genes": [{"name": "S", "sequence": bytes(aa_lut[out.aa_reference]).decode()}]})
        engine.set_schema("key", "date")
        part = engine.add_partition(N)
        engine.append_sequences(part, "main", False, 0, [bytes(row).decode() for row in nuc_lut[out.nuc]])
        engine.append_sequences(part, "S", True, 0, [bytes(row).decode() for row in aa_lut[out.aa]])
        engine.append_metadata(part, "key", "string", [str(i) for i in range(N)])
        engine.append_metadata(part, "date", "date", ["2021-03-04"] * N)
        engine.append_metadata(part, "grp", "int", [str(g) for g in group])
        engine.finalize()
    finally:
        out.lib.silo_gpu_tune(TUNE_LAUNCH_COST, 0)
    out.engine = engine
    # computed once, never changed: the exact tables per group, and what the group's query must answer at PROPORTION
    out.nuc_rows = [selected_rows(dense.mutation_counts(out.nuc, group == g, NUC_SCAN), out.nuc_reference, PROPORTION) for g in range(4)]
    out.aa_rows = [selected_rows(dense.mutation_counts(out.aa, group == g, AA_SCAN), out.aa_reference, PROPORTION) for g in range(4)]
    yield out
    engine.set_option("mutation_row_capacity", 4096)
    engine.close()


def entries(rows, reference, chars, scan, name):
    """The oracle's rows as the response lists them."""
    return [{"count": count, "mutation": f"{chars[reference[p]]}{p + 1}{chars[scan[s]]}", "proportion": count / total, "sequenceName": name}
            for p, s, count, total in rows]


def nuc_entries(made, g):
    return entries(made.nuc_rows[g], made.nuc_reference, NUC_CHARS, NUC_SCAN, "main")


def aa_entries(made, g):
    return entries(made.aa_rows[g], made.aa_reference, AA_CHARS, AA_SCAN, "S")


def query(g, action="Mutations", **fields):
    return json.dumps({"action": dict({"type": action, "minProportion": PROPORTION}, **fields),
                       "filterExpression": {"type": "IntBetween", "column": "grp", "from": g, "to": g}})


def answer(made, text):
    status, body = made.engine.execute_text(text)
    assert status == 200, body
    return body


def same_entries(body, want):
    """Counts exactly, the proportion as the parsed double equal to count / total, names and order."""
    got = json.loads(body)["queryResult"]
    assert len(got) == len(want)
    assert got == want


def blocks_of(rows):
    return {p // BLOCK for p, *_ in rows}


def test_the_stores_derive_symbols(made):
    view = made.engine.partition_store(0)
    for name, is_aa in (("main", False), ("S", True)):
        assert int(made.lib.silo_gpu_store_scan_runs(view.handle, made.engine.seqstore_id(0, name, is_aa))) > 0, name


def test_rows_in_one_finish_block_only(made):
    """(a) Group 1: the blocks 0 and 2 have no row to fence; every row is stored by threads of block 1."""
    rows = made.nuc_rows[1]
    assert blocks_of(rows) == {1} and {p for p, *_ in rows} == set(MIDDLE_ONLY)
    same_entries(answer(made, query(1)), nuc_entries(made, 1))
    assert blocks_of(made.aa_rows[1]) == {1}
    same_entries(answer(made, query(1, "AminoAcidMutations")), aa_entries(made, 1))


def test_rows_at_the_first_and_last_thread_of_every_block(made):
    """(a) Group 2: a row from thread 0 and from thread 1 023 of the blocks 0 and 1, from thread 0 and the last thread of block 2."""
    rows = made.nuc_rows[2]
    assert {p for p, *_ in rows} == set(BLOCK_EDGES)
    same_entries(answer(made, query(2)), nuc_entries(made, 2))
    assert {p for p, *_ in made.aa_rows[2]} == {0, 1_023, 1_024}
    same_entries(answer(made, query(2, "AminoAcidMutations")), aa_entries(made, 2))


def test_no_row_at_all(made):
    """(b) Group 3 is the reference: no thread stores a row, the header publishes 0."""
    assert made.nuc_rows[3] == [] and made.aa_rows[3] == []
    assert answer(made, query(3)) == b'{"queryResult":[]}'
    assert answer(made, query(3, "AminoAcidMutations")) == b'{"queryResult":[]}'
    same_entries(answer(made, query(2)), nuc_entries(made, 2))  # (and the slot's next user finds its rows)


def test_rows_in_every_block(made):
    rows = made.nuc_rows[0]
    assert blocks_of(rows) == {0, 1, 2} and {p for p, *_ in rows} >= set(BLOCK_EDGES)
    same_entries(answer(made, query(0)), nuc_entries(made, 0))
    assert blocks_of(made.aa_rows[0]) == {0, 1} and any(AA_SCAN[s] == 23 for _, s, *_ in made.aa_rows[0])  # (the stop codon among them)
    same_entries(answer(made, query(0, "AminoAcidMutations")), aa_entries(made, 0))


def test_more_rows_than_the_row_slot_holds(made):
    """(c) A slot of 4 rows: the header carries the true count and the host reads the whole table."""
    capacity = 4
    assert len(made.nuc_rows[0]) > capacity and len(made.nuc_rows[2]) > capacity and len(made.aa_rows[0]) > capacity
    made.engine.set_option("mutation_row_capacity", capacity)
    try:
        same_entries(answer(made, query(0)), nuc_entries(made, 0))
        same_entries(answer(made, query(2)), nuc_entries(made, 2))
        same_entries(answer(made, query(0, "AminoAcidMutations")), aa_entries(made, 0))
        ordered = answer(made, query(0, orderByFields=[{"field": "count", "order": "descending"}, "mutation"], limit=7, offset=3))
    finally:
        made.engine.set_option("mutation_row_capacity", 4096)
    assert ordered == answer(made, query(0, orderByFields=[{"field": "count", "order": "descending"}, "mutation"], limit=7, offset=3))


def test_two_filters_in_one_batch(made):
    """(d) Two filters of one scan, each with its slot, and the two alphabets."""
    batch = made.engine.execute_batch_text([query(0), query(2), query(1), query(3)])
    assert [status for status, _ in batch] == [200] * 4
    for (_, body), g in zip(batch, (0, 2, 1, 3)):
        same_entries(body, nuc_entries(made, g))
    batch = made.engine.execute_batch_text([query(2, "AminoAcidMutations"), query(0, "AminoAcidMutations")])
    assert [status for status, _ in batch] == [200] * 2
    for (_, body), g in zip(batch, (2, 0)):
        same_entries(body, aa_entries(made, g))


ORDERINGS = [
    dict(orderByFields=["mutation"], limit=10, offset=5),
    dict(orderByFields=[{"field": "proportion", "order": "descending"}], limit=5, offset=0),
    dict(orderByFields=[{"field": "count", "order": "ascending"}, {"field": "mutation", "order": "descending"}], limit=1_000, offset=2),
    dict(orderByFields=[{"field": "proportion", "order": "ascending"}, "count"], offset=1),
    dict(limit=3, offset=4),
    dict(limit=0),
    dict(offset=100_000),
]


def test_ordered_bodies_do_not_depend_on_where_the_rows_are_selected(made):
    """orderByFields, limit and offset: the same bytes whether the finish kernel selects (0) or the call clears, scans and selects (-1)."""
    bodies = {}
    for value in (0, -1):
        previous = made.lib.silo_gpu_tune(TUNE_FUSED_SELECT, value)
        try:
            bodies[value] = [answer(made, query(g, action, **fields))
                             for g in (0, 2) for action in ("Mutations", "AminoAcidMutations") for fields in ORDERINGS]
        finally:
            made.lib.silo_gpu_tune(TUNE_FUSED_SELECT, previous)
    assert bodies[0] == bodies[-1]
    # what the window must hold, from the oracle's rows: ordered by mutation, names are unique
    want = sorted(nuc_entries(made, 0), key=lambda entry: entry["mutation"])[5:15]
    same_entries(bodies[0][0], want)
    assert json.loads(bodies[0][4])["queryResult"] == nuc_entries(made, 0)[4:7]
    assert bodies[0][5] == bodies[0][6] == b'{"queryResult":[]}'


def test_two_filters_alternately_on_one_thread(made):
    """(e) 200 times group 0, then group 2, on the calling thread: a row that reached the host after its header would show as a
    stale or missing row of the other filter, or of the filter's last use."""
    first = [answer(made, query(0)), answer(made, query(2))]
    same_entries(first[0], nuc_entries(made, 0))
    same_entries(first[1], nuc_entries(made, 2))
    assert first[0] != first[1]
    texts = [query(0), query(2)]
    wrong = [(turn, k) for turn in range(200) for k in (0, 1) if answer(made, texts[k]) != first[k]]
    assert wrong == []
