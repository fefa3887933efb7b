"""The class-count entries of K21 (silo_gpu_distinct_count / _classes, csrc/silo_gpu_distinct_counts.hip) alone, on the numpy hash
tables of tests/test_distinct_kernels_gpu.py, against tests/distinct_counts_reference.py: the row counts around a word and 70 001
rows, row_words exact and rounded to 32, one class (the leader loop with one slot), all rows different (64 slots per wave), a probe
chain, sparse and empty filters, padding bits, the smallest table and a roomy one, one part and two with classes across the cut,
min_count around the largest class, a key list that is too short by one, and the refusals.  Every comparison is an exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import distinct_counts_reference as counts_ref  # noqa: E402
from tests.test_distinct_kernels_gpu import ALL_ONES, FILL, FILLED, KINDS, ROWS, _padded_hashes, _row_words, _words, filters, hash_table  # noqa: E402

GUARD_WORDS = 2
FILLED32 = np.uint32(0xA5A5A5A5)


def _expected_counts(owners, classes, empty):
    """uint32 [slots]: the size of the class at every owner's slot, 0 at every other slot."""
    reps = np.array(sorted(classes), dtype=np.int64)
    sizes = np.array([classes[rep] for rep in sorted(classes)], dtype=np.uint32)
    owned = owners != empty
    assert owned.sum() == len(reps) and np.array_equal(np.sort(owners[owned]), reps)
    expected = np.zeros(len(owners), dtype=np.uint32)
    expected[owned] = sizes[np.searchsorted(reps, owners[owned])]
    return expected


def _run(parts, slots, classes, min_count=1, capacity=None, calls=1):
    """One run, checked: the counts at every slot, the guards, the counter, the set of keys.  capacity None: exactly the classes."""
    from silo_amd import binding

    want = counts_ref.packed_keys(classes, min_count)
    if capacity is None:
        capacity = max(1, len(want))
    got = binding.distinct_counts(parts, slots, min_count=min_count, capacity=capacity, fill=FILL, guard_words=GUARD_WORDS, calls=calls)
    assert got["overflow"] == 0
    assert np.array_equal(got["counts"][:slots], _expected_counts(got["owners"], classes, binding.DISTINCT_EMPTY))
    assert (got["counts"][slots:] == FILLED32).all()
    assert got["n_keys"] == len(want)
    written = min(len(want), capacity)
    assert (got["keys"][written:] == FILLED).all()  # the words behind the capacity among them
    keys = np.sort(got["keys"][:written])
    if written == len(want):
        assert np.array_equal(keys, want)
    else:
        assert len(np.unique(keys)) == written and np.isin(keys, want).all()
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rounded", [False, True], ids=["exact", "rounded"])
@pytest.mark.parametrize("n", ROWS)
def test_one_part_matches_numpy(built, n, rounded, kind):
    from silo_amd import binding

    table = hash_table(kind, n)
    row_words = _row_words(n, rounded)
    hashes = _padded_hashes(table, row_words, np.random.default_rng(n))
    smallest = binding.distinct_slots(n)
    cases = [(name, mask, False) for name, mask in filters(n)] + [("padding bits", np.ones(n, dtype=bool), True)]
    for name, mask, padding_set in cases:
        classes = counts_ref.classes_by_hash(table, mask)
        assert sum(classes.values()) == int(mask.sum())
        part = dict(hashes=hashes, filter=_words(mask, row_words, padding_set), first_row=0, sequence_count=n, row_words=row_words)
        for slots in (smallest, 16 * smallest):
            _run([part], slots, classes, calls=2 if name == "half" else 1)
        if name in ("all", "half") and classes:
            largest = max(classes.values())
            for min_count in (2, largest, largest + 1):
                _run([part], smallest, classes, min_count=min_count)
            assert len(counts_ref.packed_keys(classes, largest)) >= 1 and len(counts_ref.packed_keys(classes, largest + 1)) == 0
            if len(classes) >= 2:  # a list that is too short by one: the counter still says how many classes there are
                _run([part], smallest, classes, capacity=len(classes) - 1)
    everything = counts_ref.classes_by_hash(table, np.ones(n, dtype=bool))
    if kind == "identical":
        assert everything == {0: n}
    if kind == "different":
        assert len(everything) == n
    if kind == "chain" and n == 70_001:
        assert sorted(everything.values()).count(3) == 500 and sorted(everything.values()).count(2) == 500


@pytest.mark.parametrize("kind", ["planted", "chain", "identical"])
def test_two_parts_count_the_classes_of_one(built, kind):
    """70 001 rows as one part and as 30 000 + 40 001, from row 5 of the database: the same classes, those across the cut counted
    once with the rows of both sides."""
    from silo_amd import binding

    n, cut, base = 70_001, 30_000, 5
    table = hash_table(kind, n)
    rng = np.random.default_rng(5)
    slots = binding.distinct_slots(n + base)
    for name, mask in filters(n, seed=1)[:3]:
        classes = counts_ref.classes_by_hash(table, mask, first_row=base)
        whole = dict(hashes=_padded_hashes(table, _row_words(n, True), rng), filter=_words(mask, _row_words(n, True)), first_row=base,
                     sequence_count=n, row_words=_row_words(n, True))
        one = _run([whole], slots, classes)
        parts = []
        for begin, end, rounded in ((0, cut, False), (cut, n, True)):
            row_words = _row_words(end - begin, rounded)
            parts.append(dict(hashes=_padded_hashes(table[begin:end], row_words, rng), filter=_words(mask[begin:end], row_words, True),
                              first_row=base + begin, sequence_count=end - begin, row_words=row_words))
        two = _run(parts, slots, classes, calls=2)
        assert np.array_equal(np.sort(one["keys"][:one["n_keys"]]), np.sort(two["keys"][:two["n_keys"]])), name
        _run(parts, slots, classes, min_count=2)
        if name == "all":  # not vacuous: classes with rows on both sides of the cut
            first = counts_ref.classes_by_hash(table[:cut], mask[:cut], first_row=base)
            assert any(classes[rep] > size for rep, size in first.items())


def test_refusals_write_nothing(built):
    from silo_amd import binding

    lib = binding.load_library()
    n, row_words, slots, capacity = 100, 2, 256, 8
    table = hash_table("planted", 65)
    hashes = binding._upload(np.ascontiguousarray(_padded_hashes(table, row_words, np.random.default_rng(1))))
    filter_dev = binding._upload(np.full(row_words, ALL_ONES, dtype=np.uint64))
    owners = binding.device_malloc(binding.distinct_table_bytes(slots), FILL)
    counts = binding.device_malloc(binding.distinct_counts_bytes(slots), FILL)
    keys = binding.device_malloc(capacity * 8, FILL)
    n_keys = binding.device_malloc(4, FILL)
    records = np.zeros(5, dtype=binding.DISTINCT_PART_DTYPE)
    records[0] = (hashes.value, 0, n, row_words, 0)
    records[1] = (hashes.value, 0, row_words * 64 + 1, row_words, 0)       # more rows than row words
    records[2] = (hashes.value, 2 ** 32 - 1 - n, n, row_words, 0)          # first_row + sequence_count = 2^32 - 1
    records[3] = (0, 0, n, row_words, 0)                                   # no hashes
    records[4] = (hashes.value, 0, n, 0, 0)                                # no row words
    parts = binding._upload(records)
    try:
        def count(table_dev=owners, slots=slots, counts_dev=counts, parts_dev=parts, n_parts=5, part=0, filter_dev=filter_dev):
            return lib.silo_gpu_distinct_count(table_dev, slots, counts_dev, parts_dev, n_parts, part, filter_dev, None)

        def classes(table_dev=owners, slots=slots, counts_dev=counts, parts_dev=parts, n_parts=5, part=0, filter_dev=filter_dev, min_count=1,
                    keys_dev=keys, capacity=capacity, n_keys_dev=n_keys):
            return lib.silo_gpu_distinct_classes(table_dev, slots, counts_dev, parts_dev, n_parts, part, filter_dev, min_count, keys_dev, capacity,
                                                 n_keys_dev, None)

        shared = [dict(slots=bad) for bad in (0, 3, 255, 257)] + [dict(table_dev=None), dict(counts_dev=None), dict(parts_dev=None), dict(filter_dev=None),
                                                                  dict(n_parts=0), dict(part=5), dict(part=1), dict(part=2), dict(part=3), dict(part=4)]
        for arguments in shared:
            assert count(**arguments) != 0, arguments
            assert classes(**arguments) != 0, arguments
        for arguments in (dict(keys_dev=None), dict(n_keys_dev=None), dict(capacity=0), dict(min_count=0)):
            assert classes(**arguments) != 0, arguments
        binding._check(lib.silo_gpu_stream_synchronize(None))
        assert (binding.device_read(owners, np.uint32, slots + 1) == FILLED32).all()
        assert (binding.device_read(counts, np.uint32, slots) == FILLED32).all()
        assert (binding.device_read(keys, np.uint64, capacity) == FILLED).all()
        assert (binding.device_read(n_keys, np.uint32, 1) == FILLED32).all()
    finally:
        for ptr in (hashes, filter_dev, owners, counts, keys, n_keys, parts):
            binding.device_free(ptr)
