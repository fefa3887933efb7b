"""K19 alone (silo_gpu_sample_groups / _begin / _count / _advance / _select, the kernels of the filter expression Sample) on numpy
inputs, against tests/sample_reference.py.  Every comparison is an exact equality of row-bitset words, group ids or state words."""
import numpy as np
import pytest

from tests import sample_reference as ref

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD_WORDS = 4
GUARD = np.full(GUARD_WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
SIZES = [1, 63, 64, 65, 255, 256, 257, 2049, 70_001]
INVALID_ARGUMENT = -1


def _row_words(n, rounded):
    words = (n + 63) // 64
    return (words + 31) // 32 * 32 if rounded else words


def _filters(n):
    """name -> bool [n]: all rows, a random half, 1 row in 500, one row, none."""
    rng = np.random.default_rng(100 + n)
    one = np.zeros(n, dtype=bool)
    one[int(rng.integers(0, n))] = True
    return {"all": np.ones(n, dtype=bool), "half": rng.random(n) < 0.5, "1-in-500": rng.random(n) < 0.002, "one": one, "none": np.zeros(n, dtype=bool)}


def _three_groups(n):
    rng = np.random.default_rng(200 + n)
    groups = rng.integers(0, 3, size=n).astype(np.uint16)
    groups[rng.random(n) < 0.15] = ref.NO_GROUP
    return groups


def _many_groups(n):
    """1 024 groups of very different sizes."""
    rng = np.random.default_rng(300 + n)
    return np.minimum(1023, (1024 * rng.random(n) ** 2).astype(np.int64)).astype(np.uint16)


def _part(selected, groups, row_words, first_row=0, padding_set=False):
    """A partition for binding.sample: the filter's words (with every padding bit set, if asked for) and the groups of all
    row_words * 64 rows; padding rows get group 0, so only sequence_count keeps them out."""
    n = len(selected)
    filter_words = ref.words(selected, row_words)
    if padding_set:
        filter_words = filter_words | ~ref.words(np.ones(n, dtype=bool), row_words)
    padded = None
    if groups is not None:
        padded = np.zeros(row_words * 64, dtype=np.uint16)
        padded[:n] = groups
    return {"filter": filter_words, "groups": padded, "sequence_count": n, "row_words": row_words, "first_row": first_row}


def _run(parts, size, seed, n_groups):
    from silo_amd import binding

    outputs, state = binding.sample(parts, size, seed, n_groups, fill=FILL, guard_words=GUARD_WORDS)
    for part, out in zip(parts, outputs):
        assert np.array_equal(out[part["row_words"]:], GUARD), "words past row_words were touched"
    return [out[:part["row_words"]] for part, out in zip(parts, outputs)], state


def _check_state(state, seed, size, selected, groups, n_groups, first_row=0):
    """After round 3: a group is take-all iff it has at most `size` rows; every other group has exactly one row still to take, and
    its prefix is the largest key it selects.  The histogram is clear again."""
    row_keys = ref.keys(seed, np.arange(len(selected), dtype=np.uint64) + first_row)
    assert state["n_groups"] == n_groups and state["size"] == size
    assert not state["histogram"].any()
    for group in range(n_groups):
        members = selected if groups is None else selected & (groups == group)
        if members.sum() <= size:
            assert state["take_all"][group] == 1, group
        else:
            assert state["take_all"][group] == 0 and state["remaining"][group] == 1, group
            assert state["prefix"][group] == np.sort(row_keys[members])[size - 1], group


@pytest.mark.parametrize("rounded", [False, True], ids=["exact-row-words", "row-words-rounded-to-32"])
@pytest.mark.parametrize("n", SIZES)
def test_selection_matches_the_reference(built, n, rounded):
    row_words = _row_words(n, rounded)
    seed = 2 ** 32 + 7 + n
    for name, selected in _filters(n).items():
        cardinality = int(selected.sum())
        for groups, n_groups in ((None, 1), (_three_groups(n), 3)):
            for size in sorted({0, 1, 2, max(cardinality - 1, 0), cardinality, cardinality + 1, 1000}):
                want = ref.words(ref.select(seed, size, selected, groups), row_words)
                (got,), state = _run([_part(selected, groups, row_words)], size, seed, n_groups)
                assert np.array_equal(got, want), (name, n_groups, size)
                if size >= 1:
                    _check_state(state, seed, size, selected, groups, n_groups)
    # a filter whose padding bits are all set selects the same rows
    selected = _filters(n)["half"]
    for groups, n_groups in ((None, 1), (_three_groups(n), 3)):
        for size in (1, n):
            want = ref.words(ref.select(seed, size, selected, groups), row_words)
            (got,), _ = _run([_part(selected, groups, row_words, padding_set=True)], size, seed, n_groups)
            assert np.array_equal(got, want), ("padding", n_groups, size)


def test_every_round_decides_something():
    """At 70 001 rows keys share their top 24 bits: the fourth round is needed to tell them apart."""
    row_keys = np.sort(ref.keys(2 ** 32 + 7 + 70_001, np.arange(70_001)))
    assert 50 <= int((row_keys[1:] >> 8 == row_keys[:-1] >> 8).sum()) <= 400
    assert int((row_keys[1:] >> 16 == row_keys[:-1] >> 16).sum()) >= 10_000


@pytest.mark.parametrize("size", [1, 50, 400])
def test_1024_groups(built, size):
    n = 70_001
    row_words = _row_words(n, True)
    groups = _many_groups(n)
    selected = np.random.default_rng(5).random(n) < 0.9
    sizes = np.bincount(groups[selected], minlength=1024)
    if size == 50:
        assert (sizes < size).sum() >= 100 and (sizes > size).sum() >= 100
    want = ref.select(11, size, selected, groups)
    assert want.sum() == np.minimum(sizes, size).sum()
    (got,), state = _run([_part(selected, groups, row_words)], size, 11, 1024)
    assert np.array_equal(got, ref.words(want, row_words))
    _check_state(state, 11, size, selected, groups, 1024)


@pytest.mark.parametrize("n_groups", [16, 17], ids=["histogram-in-lds", "histogram-in-global-memory"])
def test_either_side_of_the_lds_threshold(built, n_groups):
    from silo_amd import binding

    assert binding.SAMPLE_LDS_GROUPS == 16
    n = 2049
    row_words = _row_words(n, False)
    groups = np.random.default_rng(6).integers(0, n_groups, size=n).astype(np.uint16)
    selected = _filters(n)["all"]
    for size in (1, 60, 200):
        (got,), state = _run([_part(selected, groups, row_words)], size, 8, n_groups)
        assert np.array_equal(got, ref.words(ref.select(8, size, selected, groups), row_words)), size
        _check_state(state, 8, size, selected, groups, n_groups)


@pytest.mark.parametrize("strata", ["one-group", "3-groups", "1024-groups"])
def test_partitions_do_not_change_the_selection(built, strata):
    """70 001 rows in one call, and as two partitions of 30 000 + 40 001 rows whose counts add up in one histogram."""
    n, cut, seed, size = 70_001, 30_000, 1, 300 if strata != "1024-groups" else 40
    selected = _filters(n)["half"]
    groups, n_groups = {"one-group": (None, 1), "3-groups": (_three_groups(n), 3), "1024-groups": (_many_groups(n), 1024)}[strata]
    want = ref.select(seed, size, selected, groups)
    (whole,), whole_state = _run([_part(selected, groups, _row_words(n, False))], size, seed, n_groups)
    assert np.array_equal(whole, ref.words(want))
    parts = [
        _part(selected[:cut], None if groups is None else groups[:cut], _row_words(cut, False), first_row=0),
        _part(selected[cut:], None if groups is None else groups[cut:], _row_words(n - cut, True), first_row=cut),
    ]
    (first, second), state = _run(parts, size, seed, n_groups)
    assert np.array_equal(first, ref.words(want[:cut], parts[0]["row_words"]))
    assert np.array_equal(second, ref.words(want[cut:], parts[1]["row_words"]))
    for field in ("prefix", "remaining", "take_all"):
        assert np.array_equal(state[field], whole_state[field]), field
    # each partition on its own selects other rows: the histogram of both is what makes the selection global
    (alone,), _ = _run([parts[1]], size, seed, n_groups)
    assert not np.array_equal(alone, second)


def test_two_runs_give_the_same_words(built):
    n = 70_001
    row_words = _row_words(n, True)
    for groups, n_groups in ((None, 1), (_many_groups(n), 1024)):
        part = _part(_filters(n)["half"], groups, row_words)
        (first,), first_state = _run([part], 120, 3, n_groups)
        (second,), second_state = _run([part], 120, 3, n_groups)
        assert np.array_equal(first, second) and first.any()
        assert all(np.array_equal(first_state[field], second_state[field]) for field in ("prefix", "remaining", "take_all", "histogram"))


def test_the_last_rows_of_the_row_space(built):
    """first_row + sequence_count == 2^32: the largest row numbers there are."""
    n = 2049
    selected = _filters(n)["half"]
    first_row = 2 ** 32 - n
    (got,), _ = _run([_part(selected, None, _row_words(n, False), first_row=first_row)], 100, 5, 1)
    assert np.array_equal(got, ref.words(ref.select(5, 100, selected, first_row=first_row)))


def test_sample_groups_matches_numpy(built):
    from silo_amd import binding

    day = 18_000  # dates are days; 0 is NULL
    bounds = np.array([[day + 20, day + 29], [day + 10, day + 19], [0, day + 4], [day + 40, 0xFFFFFFFF], [day + 31, day + 31]], dtype=np.uint32)
    for n, rounded in ((1, False), (65, False), (257, True), (70_001, False), (70_001, True)):
        row_words = _row_words(n, rounded)
        rng = np.random.default_rng(400 + n)
        dates = (day + rng.integers(0, 50, size=row_words * 64)).astype(np.uint32)
        dates[rng.random(row_words * 64) < 0.1] = 0
        for name, selected in _filters(n).items():
            for padding_set in (False, True):
                filter_words = _part(selected, None, row_words, padding_set=padding_set)["filter"]
                got = binding.sample_groups(filter_words, dates, bounds, n, row_words, fill=FILL, guard_rows=8)
                assert (got[row_words * 64:] == 0xA5A5).all(), "groups past row_words * 64 were touched"
                want = np.full(row_words * 64, ref.NO_GROUP, dtype=np.uint16)
                want[:n] = ref.date_groups(selected, dates[:n], bounds)
                assert np.array_equal(got[:row_words * 64], want), (n, rounded, name, padding_set)
    # not vacuous, on the numpy side: every range and no range occur, both ends of a range are inclusive, NULL dates occur
    everything = ref.date_groups(np.ones(70_001, dtype=bool), dates[:70_001], bounds)
    assert set(np.unique(everything).tolist()) == {0, 1, 2, 3, 4, ref.NO_GROUP}
    assert (everything[dates[:70_001] == day + 29] == 0).all() and (everything[dates[:70_001] == day + 20] == 0).all()
    assert (everything[dates[:70_001] == day + 30] == ref.NO_GROUP).all() and (everything[dates[:70_001] == 0] == ref.NO_GROUP).all()
    assert (everything[dates[:70_001] == day + 49] == 3).all() and (everything[dates[:70_001] == day] == 2).all()


def test_refusals_write_nothing(built):
    from silo_amd import binding

    lib = binding.load_library()
    n, row_words, n_groups = 65, 2, 3
    state_bytes = binding.sample_state_bytes(n_groups)
    filter_words = ref.words(np.ones(n, dtype=bool), row_words)
    dates = np.full(row_words * 64, 18_000, dtype=np.uint32)
    bounds = np.array([[1, 17_999], [18_000, 18_000], [18_001, 0xFFFFFFFF]], dtype=np.uint32)
    state = binding.device_malloc(state_bytes, FILL)
    out = binding.device_malloc((row_words + GUARD_WORDS) * 8, FILL)
    groups = binding.device_malloc(row_words * 64 * 2, FILL)
    filter_dev, dates_dev = binding._upload(filter_words), binding._upload(dates)
    past = 2 ** 32 - n + 1  # first_row + sequence_count == 2^32 + 1

    def bounds_ptr(array):
        array = np.ascontiguousarray(array, dtype=np.uint32)
        return array, binding._ptr(array)

    try:
        good_bounds, good_ptr = bounds_ptr(bounds)
        refused = [
            lib.silo_gpu_sample_begin(None, n_groups, 10, 0, None),
            lib.silo_gpu_sample_begin(state, 0, 10, 0, None),
            lib.silo_gpu_sample_begin(state, binding.MAX_SAMPLE_GROUPS + 1, 10, 0, None),
            lib.silo_gpu_sample_begin(state, n_groups, 2 ** 31, 0, None),
            lib.silo_gpu_sample_count(None, filter_dev, None, n, row_words, 0, 0, None),
            lib.silo_gpu_sample_count(state, None, None, n, row_words, 0, 0, None),
            lib.silo_gpu_sample_count(state, filter_dev, None, n, 0, 0, 0, None),
            lib.silo_gpu_sample_count(state, filter_dev, None, row_words * 64 + 1, row_words, 0, 0, None),
            lib.silo_gpu_sample_count(state, filter_dev, None, n, row_words, 0, 4, None),
            lib.silo_gpu_sample_count(state, filter_dev, None, n, row_words, past, 0, None),
            lib.silo_gpu_sample_advance(None, 0, None),
            lib.silo_gpu_sample_advance(state, 4, None),
            lib.silo_gpu_sample_select(None, filter_dev, None, n, row_words, 0, out, None),
            lib.silo_gpu_sample_select(state, None, None, n, row_words, 0, out, None),
            lib.silo_gpu_sample_select(state, filter_dev, None, n, row_words, 0, None, None),
            lib.silo_gpu_sample_select(state, filter_dev, None, n, 0, 0, out, None),
            lib.silo_gpu_sample_select(state, filter_dev, None, row_words * 64 + 1, row_words, 0, out, None),
            lib.silo_gpu_sample_select(state, filter_dev, None, n, row_words, past, out, None),
            lib.silo_gpu_sample_groups(None, dates_dev, good_ptr, 3, n, row_words, groups, None),
            lib.silo_gpu_sample_groups(filter_dev, None, good_ptr, 3, n, row_words, groups, None),
            lib.silo_gpu_sample_groups(filter_dev, dates_dev, None, 3, n, row_words, groups, None),
            lib.silo_gpu_sample_groups(filter_dev, dates_dev, good_ptr, 3, n, row_words, None, None),
            lib.silo_gpu_sample_groups(filter_dev, dates_dev, good_ptr, 0, n, row_words, groups, None),
            lib.silo_gpu_sample_groups(filter_dev, dates_dev, good_ptr, 3, n, 0, groups, None),
            lib.silo_gpu_sample_groups(filter_dev, dates_dev, good_ptr, 3, row_words * 64 + 1, row_words, groups, None),
        ]
        many, many_ptr = bounds_ptr([[2 * k + 1, 2 * k + 1] for k in range(binding.MAX_SAMPLE_GROUPS + 1)])
        refused.append(lib.silo_gpu_sample_groups(filter_dev, dates_dev, many_ptr, len(many), n, row_words, groups, None))
        backwards, backwards_ptr = bounds_ptr([[1, 10], [30, 20]])
        refused.append(lib.silo_gpu_sample_groups(filter_dev, dates_dev, backwards_ptr, 2, n, row_words, groups, None))
        overlapping, overlapping_ptr = bounds_ptr([[20, 30], [1, 20]])
        refused.append(lib.silo_gpu_sample_groups(filter_dev, dates_dev, overlapping_ptr, 2, n, row_words, groups, None))
        assert refused == [INVALID_ARGUMENT] * len(refused), refused
        binding._check(lib.silo_gpu_stream_synchronize(None))
        assert (binding.device_read(state, np.uint8, state_bytes) == FILL).all()
        assert (binding.device_read(out, np.uint8, (row_words + GUARD_WORDS) * 8) == FILL).all()
        assert (binding.device_read(groups, np.uint8, row_words * 64 * 2) == FILL).all()
        # the same buffers serve good calls
        binding._check(lib.silo_gpu_sample_groups(filter_dev, dates_dev, good_ptr, 3, n, row_words, groups, None))
        assert np.array_equal(binding.device_read(groups, np.uint16, row_words * 64), np.where(np.arange(row_words * 64) < n, 1, ref.NO_GROUP))
        binding._check(lib.silo_gpu_sample_begin(state, n_groups, 10, 0, None))
        for sample_round in range(binding.SAMPLE_ROUNDS):
            binding._check(lib.silo_gpu_sample_count(state, filter_dev, groups, n, row_words, 0, sample_round, None))
            binding._check(lib.silo_gpu_sample_advance(state, sample_round, None))
        binding._check(lib.silo_gpu_sample_select(state, filter_dev, groups, n, row_words, 0, out, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        got = binding.device_read(out, np.uint64, row_words + GUARD_WORDS)
        assert np.array_equal(got[:row_words], ref.words(ref.select(0, 10, np.ones(n, dtype=bool)), row_words)) and np.array_equal(got[row_words:], GUARD)
    finally:
        for ptr in (state, out, groups, filter_dev, dates_dev):
            binding.device_free(ptr)
