"""The filter compiler (ProgramBuilder and the operators' lower()) at and beyond the limits of one device program: 128 leaves, 320
instructions, 32 slots.  Wide Or / And / N-Of nodes, many composite children and deep nesting, on a synthetic store of
8 193 + 64 + 1 rows, through Aggregated (count only), Details (the bitset) and the engine's batch call, against numpy on the raw
symbol matrix -- and, for Maybe / Exact / HasNucleotideMutation, against the CPU oracle on the first rows of the same data."""
import json
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import silo_oracle as so  # noqa: E402

NUC_CHARS = "-ACGTRYSWKMBDHVN"
PARTITIONS = [8193, 1, 64]  # 8 192 rows are one 128-word tile of the evaluators
N_ROWS = sum(PARTITIONS)
POSITIONS = 400
ORACLE_ROWS = 300
WIDTHS = (127, 128, 129, 200, 300)


# ---- data ----------------------------------------------------------------------------------------------------------------------
class World:
    """The symbol matrix, leaf pools by frequency, and the cases built from them (expression, expected row mask)."""

    def __init__(self):
        rng = np.random.default_rng(20261020)
        self.reference = 1 + (np.arange(POSITIONS) % 4)
        kind = np.zeros(POSITIONS, dtype=int)  # 0: conserved (300 positions), 1: medium (40), 2: variable (60)
        shuffled = rng.permutation(POSITIONS)
        kind[shuffled[:40]] = 1
        kind[shuffled[40:100]] = 2
        # per cell: another of "-ACGT" / N / an IUPAC code; else the reference symbol (0.93 of all cells, N 0.7 %, IUPAC 0.5 %)
        p_other = np.array([0.001, 0.04, 0.34])[kind]
        p_n = np.array([0.001, 0.005, 0.04])[kind]
        p_iupac = np.array([0.001, 0.01, 0.02])[kind]
        u = rng.random((N_ROWS, POSITIONS))
        alternatives = np.array([rng.permutation([s for s in range(5) if s != r]) for r in self.reference])
        which = rng.choice(4, p=[0.5, 0.3, 0.15, 0.05], size=(N_ROWS, POSITIONS))
        other = alternatives[np.arange(POSITIONS)[None, :], which]
        sym = np.broadcast_to(self.reference, (N_ROWS, POSITIONS)).copy()
        is_other = u < p_other
        is_n = ~is_other & (u < p_other + p_n)
        is_iupac = ~is_other & ~is_n & (u < p_other + p_n + p_iupac)
        sym[is_other] = other[is_other]
        sym[is_n] = 15
        sym[is_iupac] = rng.integers(5, 15, size=int(is_iupac.sum()))
        self.sym = sym.astype(np.uint8)
        self.kind = kind
        self.frequency = np.stack([(self.sym == s).mean(axis=0) for s in range(16)], axis=1)  # [position, symbol]
        self.conserved_ref = [(int(p), int(self.reference[p])) for p in np.flatnonzero(kind == 0)]
        self.variable_ref = [(int(p), int(self.reference[p])) for p in np.flatnonzero(kind == 2)]
        self.variable_alt = [(int(p), int(s)) for p in np.flatnonzero(kind == 2) for s in alternatives[p]]
        non_reference = [(p, s) for p in range(POSITIONS) for s in range(16) if s != self.reference[p] and self.frequency[p, s] > 0]
        self.rare = sorted(non_reference, key=lambda leaf: (-self.frequency[leaf], leaf))
        self.cases = {}
        self.masks = {}

    def rarest(self, count, budget, skip=()):
        """`count` non-reference leaves, the most frequent whose frequencies stay at or below budget / count each: the union
        of all of them selects roughly 1 - exp(-budget) of the rows."""
        taken = [leaf for leaf in self.rare if self.frequency[leaf] <= budget / count and leaf not in skip][:count]
        assert len(taken) == count
        return taken

    def leaf_mask(self, leaf):
        if leaf not in self.masks:
            self.masks[leaf] = self.sym[:, leaf[0]] == leaf[1]
        return self.masks[leaf]

    def evaluate(self, expression, rows=N_ROWS):
        """Plain numpy on the raw symbols: the reference of every case without ambiguity."""
        kind = expression["type"]
        if kind == "NucleotideEquals":
            return self.leaf_mask((expression["position"] - 1, NUC_CHARS.index(expression["symbol"])))[:rows]
        if kind == "IntBetween":
            index = np.arange(rows)
            return (index >= expression["from"]) & (index <= expression["to"])
        if kind == "Not":
            return ~self.evaluate(expression["child"], rows)
        children = [self.evaluate(child, rows) for child in expression["children"]]
        if kind == "And":
            return np.logical_and.reduce(children)
        if kind == "Or":
            return np.logical_or.reduce(children)
        assert kind == "N-Of"
        matches = np.sum(children, axis=0)  # identical children count once each
        return matches == expression["numberOfMatchers"] if expression["matchExactly"] else matches >= expression["numberOfMatchers"]

    def n_of(self, children, exactly):
        """N-Of with n picked from the numpy per-row match counts: the commonest count for 'exactly', the median for 'at least'."""
        matches = np.sum([self.evaluate(child) for child in children], axis=0)
        n = int(np.bincount(matches).argmax()) if exactly else int(np.quantile(matches, 0.5, method="lower"))
        n = min(max(n, 1), len(children) - 1)
        return {"type": "N-Of", "numberOfMatchers": n, "matchExactly": exactly, "children": children}

    def case(self, name):
        if name not in self.cases:
            kind, _, argument = name.partition("-")
            expression = BUILDERS[kind](self, np.random.default_rng(sum(name.encode())), int(argument or 0))
            self.cases[name] = (expression, self.evaluate(expression))
        return self.cases[name]


def equals(leaf):
    return {"type": "NucleotideEquals", "position": leaf[0] + 1, "symbol": NUC_CHARS[leaf[1]]}


def negate_odd(children):
    return [child if i % 2 == 0 else {"type": "Not", "child": child} for i, child in enumerate(children)]


def counted_leaves(world, rng, width):
    """`width` distinct leaves whose per-row match count spreads over a few values: 12 reference symbols at variable positions,
    the rest conserved reference symbols and rare symbols."""
    variable = [world.variable_ref[i] for i in rng.permutation(len(world.variable_ref))[:12]]
    rest = world.conserved_ref[:(width - 12) // 2]
    return variable + rest + world.rarest(width - 12 - len(rest), 2.0)


# shapes 1 and 2: flat nodes of `width` distinct leaves, plain and with every second child under Not
def flat_or(world, rng, width):
    return {"type": "Or", "children": [equals(leaf) for leaf in world.rarest(width, 0.8)]}


def flat_and(world, rng, width):
    return {"type": "And", "children": [equals(leaf) for leaf in world.conserved_ref[:width]]}


def flat_at_least(world, rng, width):
    return world.n_of([equals(leaf) for leaf in counted_leaves(world, rng, width)], False)


def flat_exactly(world, rng, width):
    return world.n_of([equals(leaf) for leaf in counted_leaves(world, rng, width)], True)


def half_negated_or(world, rng, width):  # Not of a conserved reference symbol is as rare as the rare symbols
    leaves = [leaf for pair in zip(world.rarest(width, 0.4), world.conserved_ref) for leaf in pair][:width]
    return {"type": "Or", "children": negate_odd([equals(leaf) for leaf in leaves])}


def half_negated_and(world, rng, width):
    leaves = [leaf for pair in zip(world.conserved_ref, world.rarest(width, 0.4)) for leaf in pair][:width]
    return {"type": "And", "children": negate_odd([equals(leaf) for leaf in leaves])}


def half_negated_at_least(world, rng, width):
    return world.n_of(negate_odd([equals(leaf) for leaf in counted_leaves(world, rng, width)]), False)


def half_negated_exactly(world, rng, width):
    return world.n_of(negate_odd([equals(leaf) for leaf in counted_leaves(world, rng, width)]), True)


# shape 3: leafRun does not de-duplicate, leaf() does
def repeated_leaf(world, rng, _):
    children = [equals(leaf) for leaf in counted_leaves(world, rng, 150)] + [equals(world.variable_ref[20])] * 50
    return world.n_of(children, False)


# shape 4: many composite children
def or_of_ands(world, rng, count):
    rare = world.rarest(count, 0.8)
    return {"type": "Or", "children": [{"type": "And", "children": [equals(world.conserved_ref[i]), equals(rare[i])]} for i in range(count)]}


def n_of_ors(world, rng, count):
    rare = world.rarest(count, 2.0)
    alt = [world.variable_alt[i] for i in rng.permutation(len(world.variable_alt))]
    children = [{"type": "Or", "children": [equals(rare[i]), equals(alt[i % 24])]} for i in range(count)]
    return world.n_of(children, False)


# shape 5: wide nodes below the root
def wide_below_root(world, rng, _):
    wide_or = {"type": "Or", "children": [equals(leaf) for leaf in world.rarest(200, 0.4)]}
    return {"type": "And", "children": [
        {"type": "IntBetween", "column": "row", "from": N_ROWS // 10, "to": N_ROWS - N_ROWS // 10},
        {"type": "Not", "child": wide_or},
        world.n_of([equals(leaf) for leaf in counted_leaves(world, rng, 150)], False)]}


# shapes 6 and 7: the instruction limit
def or_of_triples(world, rng, count):  # 30 distinct leaves: the leaf limit is not what trips
    pool = [world.variable_alt[i] for i in rng.permutation(len(world.variable_alt))[:30]]
    children = []
    for _ in range(count):
        a, b, c = (pool[i] for i in rng.choice(30, size=3, replace=False))
        children.append({"type": "And", "children": [equals(a), {"type": "Not", "child": equals(b)}, equals(c)]})
    return {"type": "Or", "children": children}


def negated_composites(world, rng, count):
    pool = world.variable_alt + world.variable_ref
    children = []
    for _ in range(count):
        a, b = (pool[i] for i in rng.choice(len(pool), size=2, replace=False))
        children.append({"type": "Not", "child": {"type": "And", "children": [equals(a), equals(b)]}})
    return world.n_of(children, False)


# shapes 8 and 9: the slot limit
def nested_n_of(world, rng, depth):
    pool = [world.variable_ref[i] for i in rng.permutation(len(world.variable_ref))]
    leaves = iter(pool + world.variable_alt)
    node = equals(next(leaves))
    for _ in range(depth):
        node = {"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [node] + [equals(next(leaves)) for _ in range(3)]}
    return node


def alternation(world, rng, depth, columns=1):
    """And(x.., Or(y.., And(...))): `depth` nested nodes, each with `columns` leaves of its own."""
    conserved, rare = iter(world.conserved_ref), iter(world.rarest(200, 0.4))
    node = equals(world.variable_ref[3])
    for level in range(depth):
        if (depth - level) % 2 == 1:  # the outermost node is an And
            node = {"type": "And", "children": [equals(next(conserved)) for _ in range(columns)] + [node]}
        else:
            node = {"type": "Or", "children": [equals(next(rare)) for _ in range(columns)] + [node]}
    return node


def alternation_of_pairs(world, rng, depth):  # two leaves per node: every open And / Or keeps its accumulator in a slot
    return alternation(world, rng, depth, columns=2)


def fragmented_slots(world, rng, depth):
    """The slot estimate counts live slots, the allocator takes the first free run.  Below `depth` nested 4-child N-Ofs (3 counter
    slots each) sits Or(N-Of of 4, N-Of of 16): with 24 slots taken the first N-Of leaves its result above a hole of 3, the
    5-slot counter of the second fits neither the hole nor the 4 slots above it although 7 are free, and the compiler has to
    take that child out of the program again."""
    leaves = iter([world.variable_ref[i] for i in rng.permutation(len(world.variable_ref))] + world.variable_alt)
    small = {"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [equals(next(leaves)) for _ in range(4)]}
    node = {"type": "Or", "children": [small, world.n_of([equals(next(leaves)) for _ in range(16)], False)]}
    for _ in range(depth):
        node = {"type": "N-Of", "numberOfMatchers": 2, "matchExactly": False, "children": [node] + [equals(next(leaves)) for _ in range(3)]}
    return node


BUILDERS = {
    "or": flat_or, "and": flat_and, "atleast": flat_at_least, "exactly": flat_exactly,
    "or_half_negated": half_negated_or, "and_half_negated": half_negated_and, "atleast_half_negated": half_negated_at_least,
    "exactly_half_negated": half_negated_exactly, "repeated_leaf": repeated_leaf, "or_of_ands": or_of_ands, "n_of_ors": n_of_ors,
    "wide_below_root": wide_below_root, "or_of_triples": or_of_triples, "negated_composites": negated_composites,
    "nested_n_of": nested_n_of, "alternation": alternation, "alternation_of_pairs": alternation_of_pairs,
    "fragmented_slots": fragmented_slots,
}
CASES = (
    [f"{kind}-{width}" for kind in list(BUILDERS)[:8] for width in WIDTHS]
    + ["repeated_leaf"]
    + [f"{kind}-{count}" for kind in ("or_of_ands", "n_of_ors") for count in (63, 64, 65, 70, 150)]
    + ["wide_below_root", "or_of_triples-110", "negated_composites-120"]
    + [f"nested_n_of-{depth}" for depth in (8, 10, 11, 12, 20)]
    + [f"{kind}-{depth}" for kind in ("alternation", "alternation_of_pairs") for depth in (30, 33, 40)]
    + ["fragmented_slots-8"]
)


@pytest.fixture(scope="module")
def world():
    return World()


def build_engine(world, sizes, rows=N_ROWS):
    from silo_amd.engine import Engine

    reference = "".join(NUC_CHARS[s] for s in world.reference)
    engine = Engine({"nucleotideSequences": [{"name": "main", "sequence": reference}], "genes": []})
    engine.set_schema("key")
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    assert sum(sizes) == rows
    lo = 0
    for size in sizes:
        part = engine.add_partition(size)
        engine.append_sequences(part, "main", False, 0, [bytes(row).decode() for row in lut[world.sym[lo:lo + size]]])
        engine.append_metadata(part, "key", "string", [str(i) for i in range(lo, lo + size)])
        engine.append_metadata(part, "row", "int", [str(i) for i in range(lo, lo + size)])
        lo += size
    engine.finalize()
    return engine


@pytest.fixture(scope="module", params=[[N_ROWS], PARTITIONS], ids=["1-partition", "3-partitions"])
def engine(request, built, world):
    engine = build_engine(world, request.param)
    yield engine
    engine.close()


ORDINARY = [
    {"type": "NucleotideEquals", "position": 7, "symbol": "N"},
    {"type": "And", "children": [{"type": "IntBetween", "column": "row", "from": 100, "to": 8200},
                                 {"type": "Not", "child": {"type": "NucleotideEquals", "position": 11, "symbol": "-"}}]},
]


def aggregated(expression):
    return {"action": {"type": "Aggregated"}, "filterExpression": expression}


def details(expression):
    return {"action": {"type": "Details", "fields": ["key"]}, "filterExpression": expression}


def check_all_entry_paths(engine, expression, expected_keys, ordinary):
    """The three ways a program reaches the device: count only, the bitset, and the batch between two ordinary queries."""
    assert engine.execute_query(aggregated(expression)) == [{"count": len(expected_keys)}]
    rows = engine.execute_query(details(expression))
    assert len(rows) == len(expected_keys) and {row["key"] for row in rows} == expected_keys
    batch = engine.execute_batch([aggregated(ordinary[0][0]), aggregated(expression), aggregated(ordinary[1][0])])
    assert [(status, document.get("queryResult")) for status, document in batch] == [
        (200, [{"count": ordinary[0][1]}]), (200, [{"count": len(expected_keys)}]), (200, [{"count": ordinary[1][1]}])]


# ---- numpy-checked shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_wide_and_deep_filters_match_numpy(engine, world, name):
    expression, mask = world.case(name)
    count = int(mask.sum())
    assert 0.05 * N_ROWS < count < 0.95 * N_ROWS, f"{name}: the reference selects {count} of {N_ROWS} rows, which proves nothing"
    ordinary = [(e, int(world.evaluate(e).sum())) for e in ORDINARY]
    assert all(0 < c < N_ROWS for _, c in ordinary)
    check_all_entry_paths(engine, expression, {str(i) for i in np.flatnonzero(mask)}, ordinary)


def test_wide_or_twice_and_from_two_threads(engine, world):
    """A wide Or leaves its partial results in pooled temporaries: they must not return to the pool while a launch still reads
    them, so the same query twice in a row, and from two threads at once (every thread draws from the same pool), agrees."""
    expression, mask = world.case("or-300")
    other, other_mask = world.case("or_of_ands-150")
    want = [[{"count": int(mask.sum())}], [{"count": int(other_mask.sum())}]]
    assert [engine.execute_query(aggregated(expression)) for _ in range(2)] == [want[0], want[0]]
    results = [[], []]

    def client(index):
        for k in range(6):
            query = (expression, other)[(index + k) % 2]
            results[index].append(engine.execute_raw(aggregated(query) if k % 3 else details(query)))

    threads = [threading.Thread(target=client, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    keys = [{str(i) for i in np.flatnonzero(m)} for m in (mask, other_mask)]
    for index in range(2):
        assert len(results[index]) == 6
        for k, (status, document) in enumerate(results[index]):
            which = (index + k) % 2
            assert status == 200
            rows = document["queryResult"]
            if k % 3:
                assert rows == want[which]
            else:
                assert len(rows) == len(keys[which]) and {row["key"] for row in rows} == keys[which]


# ---- oracle-checked shapes: Maybe / Exact / HasNucleotideMutation ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(built, world):
    """The first ORACLE_ROWS rows of the same data: an engine in three partitions and the CPU oracle's database."""
    engine = build_engine(world, [257, 1, 42], ORACLE_ROWS)
    database = so.Database({"main": [int(s) for s in world.reference]}, {})
    database.set_config([("key", "string"), ("row", "int")], "key")
    lut = np.frombuffer(NUC_CHARS.encode(), dtype=np.uint8)
    partition = database.add_partition({"main": [bytes(row).decode() for row in lut[world.sym[:ORACLE_ROWS]]]}, {})
    database.add_metadata(partition, [{"key": str(i), "row": str(i)} for i in range(ORACLE_ROWS)])
    yield engine, database
    engine.close()


def ambiguous_cases(world):
    rng = np.random.default_rng(5)
    spread = [equals(leaf) for leaf in counted_leaves(world, rng, 150)]
    exactly = world.n_of(spread, True)
    mutated = [{"type": "HasNucleotideMutation", "position": int(p) + 1} for p in np.flatnonzero(world.kind > 0)] + [
        {"type": "HasNucleotideMutation", "position": leaf[0] + 1} for leaf in world.conserved_ref[:50]]
    return {
        "maybe_exactly-150": {"type": "Maybe", "child": exactly},
        "exact_exactly-150": {"type": "Exact", "child": exactly},
        "mutated_at_least-150": {"type": "N-Of", "numberOfMatchers": 48, "matchExactly": False, "children": mutated},
    }


@pytest.mark.parametrize("name", ["maybe_exactly-150", "exact_exactly-150", "mutated_at_least-150"])
def test_wide_ambiguous_filters_match_the_oracle(small, world, name):
    engine, database = small
    expression = ambiguous_cases(world)[name]
    expected = {row["key"] for row in json.loads(json.dumps(so.execute_query(database, details(expression))))}
    assert 0.05 * ORACLE_ROWS < len(expected) < 0.95 * ORACLE_ROWS, f"{name}: the oracle selects {len(expected)} of {ORACLE_ROWS} rows"
    ordinary = [(e, so.execute_query(database, aggregated(e))[0]["count"]) for e in ORDINARY[:1] * 2]
    check_all_entry_paths(engine, expression, expected, ordinary)
