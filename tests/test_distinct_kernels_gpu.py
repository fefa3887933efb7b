"""The selection entries of K20 (silo_gpu_distinct_begin / _insert / _select, csrc/silo_gpu_distinct.hip) alone, on tables of hashes
made in numpy, against tests/distinct_reference.py: the row counts around a word and 70 001 rows, row_words exact and rounded to 32,
classes of every size, a probe chain of 1 000 classes with one home slot, hashes that differ in one lane only, sparse and empty
filters, padding bits, the smallest table and a roomy one, one part and two with classes across the cut, and the refusals.  Every
comparison is an exact equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import distinct_reference as ref  # noqa: E402

FILL = 0xA5
FILLED = np.uint64(0xA5A5A5A5A5A5A5A5)
ROWS = [1, 63, 64, 65, 70_001]
KINDS = ["identical", "different", "planted", "chain", "lane1"]
GUARD_WORDS = 2
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _row_words(n, rounded):
    words = -(-n // 64)
    return -(-words // 32) * 32 if rounded else words


@functools.lru_cache(maxsize=None)
def hash_table(kind, n):
    """uint64 [n][2].  identical: one class.  different: n classes.  planted: classes of 2, 3, 5, ... up to 5 000 rows scattered
    over the table among rows that are alone.  chain: up to 1 000 different hashes that share the low 26 bits of lane 0 — one home
    slot in every table of this file — each held by one to three rows.  lane1: groups of rows equal in lane 0 that differ in lane
    1, and pairs equal in both."""
    rng = np.random.default_rng(1200 + n + 17 * KINDS.index(kind))
    table = rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 2), dtype=np.uint64)
    order = rng.permutation(n)
    if kind == "identical":
        table[:] = table[0]
    elif kind == "planted":
        start = 0
        for size in (2, 3, 5, 64, 65, 700, 5000):
            if start + size > n * 3 // 4:
                break
            table[order[start:start + size]] = table[order[start]]
            start += size
    elif kind == "chain":
        classes = min(1000, n)
        low = np.uint64(0x2ABCDEF)  # < 2^26
        heads = order[:classes]
        table[heads, 0] = (table[heads, 0] & ~np.uint64((1 << 26) - 1)) | low
        copies = order[classes:classes + min(classes, n - classes)]
        table[copies] = table[heads[:len(copies)]]
        more = order[2 * classes:2 * classes + min(classes // 2, max(0, n - 2 * classes))]
        table[more] = table[heads[:len(more)]]
    elif kind == "lane1":
        for group in range(min(50, n // 6)):
            rows = order[6 * group:6 * group + 6]
            table[rows, 0] = table[rows[0], 0]
            table[rows[5]] = table[rows[4]]
    table.setflags(write=False)
    return table


def filters(n, seed=0):
    """(name, bool [n]) — all rows, a half, 1 in 500, one row, none."""
    rng = np.random.default_rng(1300 + n + seed)
    one = np.zeros(n, dtype=bool)
    one[int(rng.integers(0, n))] = True
    sparse = rng.random(n) < 1 / 500
    return [("all", np.ones(n, dtype=bool)), ("half", rng.random(n) < 0.5), ("1 in 500", sparse), ("one", one), ("none", np.zeros(n, dtype=bool))]


def _words(mask, row_words, padding_set=False):
    padded = np.full(row_words * 64, padding_set, dtype=bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


def _padded_hashes(table, row_words, rng):
    """The table with rows behind it that no entry may read as rows: copies of real hashes, so that a read would show."""
    padded = np.zeros((row_words * 64, 2), dtype=np.uint64)
    padded[:len(table)] = table
    if len(padded) > len(table):
        padded[len(table):] = table[rng.integers(0, len(table), size=len(padded) - len(table))]
    return padded


def _run(parts, slots, calls=1):
    from silo_amd import binding

    outputs, owners, overflow = binding.distinct(parts, slots, fill=FILL, guard_words=GUARD_WORDS, calls=calls)
    assert overflow == 0
    for part, out in zip(parts, outputs):
        assert (out[part["row_words"]:] == FILLED).all()
    return [out[:part["row_words"]] for part, out in zip(parts, outputs)], owners


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rounded", [False, True], ids=["exact", "rounded"])
@pytest.mark.parametrize("n", ROWS)
def test_one_part_matches_numpy(built, n, rounded, kind):
    from silo_amd import binding

    table = hash_table(kind, n)
    row_words = _row_words(n, rounded)
    rng = np.random.default_rng(n)
    hashes = _padded_hashes(table, row_words, rng)
    smallest = binding.distinct_slots(n)
    assert smallest >= 2 * n and smallest // 2 < 2 * n and smallest <= 1 << 26
    cases = [(name, mask, False) for name, mask in filters(n)] + [("padding bits", np.ones(n, dtype=bool), True)]
    for name, mask, padding_set in cases:
        want = ref.select_by_hash(table, mask)
        for slots in (smallest, 16 * smallest):
            part = dict(hashes=hashes, filter=_words(mask, row_words, padding_set), first_row=0, sequence_count=n, row_words=row_words)
            (got,), owners = _run([part], slots, calls=2 if name == "half" else 1)
            assert np.array_equal(got, _words(want, row_words)), (name, slots)
            assert np.array_equal(np.sort(owners[owners != binding.DISTINCT_EMPTY]), np.flatnonzero(want)), (name, slots)
    if kind == "identical":
        assert ref.select_by_hash(table, np.ones(n, dtype=bool)).sum() == 1
    if kind == "different":
        assert ref.select_by_hash(table, np.ones(n, dtype=bool)).sum() == n
    if n == 70_001:
        everything = ref.select_by_hash(table, np.ones(n, dtype=bool))
        if kind == "planted":
            assert n - everything.sum() == 1 + 2 + 4 + 63 + 64 + 699 + 4999
        if kind == "chain":
            assert len(np.unique(table[:, 0] & np.uint64((1 << 26) - 1))) < n - 900 and n - everything.sum() == 1500
        if kind == "lane1":
            assert n - everything.sum() == 50 and len(np.unique(table[:, 0])) == n - 250


@pytest.mark.parametrize("kind", ["planted", "chain", "identical"])
def test_two_parts_select_the_rows_of_one(built, kind):
    """70 001 rows as one part and as 30 000 + 40 001: the same rows of the database, a class across the cut represented in the
    earlier part; parts that begin at row 5 of the database, not at 0."""
    from silo_amd import binding

    n, cut, base = 70_001, 30_000, 5
    table = hash_table(kind, n)
    rng = np.random.default_rng(5)
    slots = binding.distinct_slots(n + base)
    for name, mask in filters(n, seed=1)[:3]:
        want = ref.select_by_hash(table, mask)
        whole = dict(hashes=_padded_hashes(table, _row_words(n, True), rng), filter=_words(mask, _row_words(n, True)), first_row=base,
                     sequence_count=n, row_words=_row_words(n, True))
        (one,), _ = _run([whole], slots)
        assert np.array_equal(one, _words(want, whole["row_words"])), name
        parts = []
        for begin, end, rounded in ((0, cut, False), (cut, n, True)):
            row_words = _row_words(end - begin, rounded)
            parts.append(dict(hashes=_padded_hashes(table[begin:end], row_words, rng), filter=_words(mask[begin:end], row_words, True),
                              first_row=base + begin, sequence_count=end - begin, row_words=row_words))
        (first, second), owners = _run(parts, slots)
        assert np.array_equal(first, _words(want[:cut], parts[0]["row_words"])), name
        assert np.array_equal(second, _words(want[cut:], parts[1]["row_words"])), name
        assert np.array_equal(np.sort(owners[owners != binding.DISTINCT_EMPTY]), np.flatnonzero(want) + base), name
        if name == "all":  # not vacuous: classes with rows on both sides of the cut, whose later rows are not selected
            _, class_of_row = np.unique(table, axis=0, return_inverse=True)
            class_of_row = class_of_row.reshape(-1)
            across = np.intersect1d(class_of_row[:cut], class_of_row[cut:])
            assert len(across) >= 1 and not want[cut:][np.isin(class_of_row[cut:], across)].any()


def test_refusals_write_nothing(built):
    from silo_amd import binding

    lib = binding.load_library()
    n, row_words, slots = 100, 2, 256
    table = hash_table("planted", 65)
    hashes = binding._upload(np.ascontiguousarray(_padded_hashes(table, row_words, np.random.default_rng(1))))
    filter_dev = binding._upload(np.full(row_words, ALL_ONES, dtype=np.uint64))
    owners = binding.device_malloc(binding.distinct_table_bytes(slots), FILL)
    out = binding.device_malloc(row_words * 8, FILL)
    records = np.zeros(5, dtype=binding.DISTINCT_PART_DTYPE)
    records[0] = (hashes.value, 0, n, row_words, 0)
    records[1] = (hashes.value, 0, row_words * 64 + 1, row_words, 0)       # more rows than row words
    records[2] = (hashes.value, 2 ** 32 - 1 - n, n, row_words, 0)          # first_row + sequence_count = 2^32 - 1
    records[3] = (0, 0, n, row_words, 0)                                   # no hashes
    records[4] = (hashes.value, 0, n, 0, 0)                                # no row words
    parts = binding._upload(records)
    last = np.zeros(1, dtype=binding.DISTINCT_PART_DTYPE)
    last[0] = (hashes.value, 2 ** 32 - 2 - n, n, row_words, 0)             # the largest row numbers there can be
    last_part = binding._upload(last)
    try:
        assert lib.silo_gpu_distinct_begin(None, slots, None) != 0
        for bad_slots in (0, 3, 255, 257):
            assert lib.silo_gpu_distinct_begin(owners, bad_slots, None) != 0
            assert lib.silo_gpu_distinct_insert(owners, bad_slots, parts, 5, 0, filter_dev, None) != 0
            assert lib.silo_gpu_distinct_select(owners, bad_slots, parts, 5, 0, filter_dev, out, None) != 0
        for arguments in ((None, slots, parts, 5, 0, filter_dev), (owners, slots, None, 5, 0, filter_dev), (owners, slots, parts, 5, 0, None),
                          (owners, slots, parts, 0, 0, filter_dev), (owners, slots, parts, 5, 5, filter_dev), (owners, slots, parts, 5, 1, filter_dev),
                          (owners, slots, parts, 5, 2, filter_dev), (owners, slots, parts, 5, 3, filter_dev), (owners, slots, parts, 5, 4, filter_dev)):
            assert lib.silo_gpu_distinct_insert(*arguments, None) != 0, arguments
            assert lib.silo_gpu_distinct_select(*arguments, out, None) != 0, arguments
        assert lib.silo_gpu_distinct_select(owners, slots, parts, 5, 0, filter_dev, None, None) != 0
        binding._check(lib.silo_gpu_stream_synchronize(None))
        assert (binding.device_read(owners, np.uint32, slots + 1) == 0xA5A5A5A5).all()
        assert (binding.device_read(out, np.uint64, row_words) == FILLED).all()
        # ... and a part that is in order is taken, up to the largest row numbers there can be
        binding._check(lib.silo_gpu_distinct_begin(owners, slots, None))
        binding._check(lib.silo_gpu_distinct_insert(owners, slots, last_part, 1, 0, filter_dev, None))
        binding._check(lib.silo_gpu_distinct_select(owners, slots, last_part, 1, 0, filter_dev, out, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        want = ref.select_by_hash(_padded_hashes(table, row_words, np.random.default_rng(1))[:n], np.ones(n, dtype=bool))
        assert np.array_equal(binding.device_read(out, np.uint64, row_words), _words(want, row_words))
        words = binding.device_read(owners, np.uint32, slots + 1)
        assert words[slots] == 0 and np.array_equal(np.sort(words[:slots][words[:slots] != binding.DISTINCT_EMPTY]), np.flatnonzero(want) + (2 ** 32 - 2 - n))
    finally:
        for ptr in (hashes, filter_dev, owners, out, parts, last_part):
            binding.device_free(ptr)
