"""The numpy reference of Sample (tests/sample_reference.py) against the known answers of its definition, and the properties the
engine's tests rely on: no two rows share a key, samples are nested in their size, spread over the row range and independent
between seeds.  Runs anywhere: the host function of the library (silo_gpu_sample_key) needs no device either."""
import numpy as np
import pytest

from tests import sample_reference as ref

SEEDS = range(20)
N_ROWS = 100_000
SIZE = 1_000
_SAMPLES = {}


def _sample(seed):
    """The rows of a sample of SIZE of N_ROWS rows (computed once per seed, never changed)."""
    if seed not in _SAMPLES:
        rows = np.flatnonzero(ref.select(seed, SIZE, np.ones(N_ROWS, dtype=bool)))
        rows.setflags(write=False)
        _SAMPLES[seed] = rows
    return _SAMPLES[seed]


def test_known_answers():
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF
    assert ref.keys(0, range(4)).tolist() == [0x59E7DC65, 0xEB8818AA, 0xD30AA1F6, 0x04F78CC2]
    assert ref.keys(1, range(4)).tolist() == [0x73FD2E51, 0x2B5768EA, 0x7D07F00D, 0xE2DD0F24]
    assert ref.keys(2 ** 32 + 7, range(4)).tolist() == [0x4815CAD3, 0x41FEC33F, 0x516A7103, 0xDA8ED406]
    everything = np.ones(100, dtype=bool)
    assert np.flatnonzero(ref.select(0, 10, everything)).tolist() == [3, 4, 14, 23, 24, 40, 60, 86, 90, 91]
    assert np.flatnonzero(ref.select(1, 10, everything)).tolist() == [21, 25, 29, 38, 51, 59, 65, 76, 80, 87]


def test_the_library_computes_the_same_keys(built):
    from silo_amd import binding

    rows = [0, 1, 2, 3, 99, 2 ** 24, 2 ** 31, 2 ** 32 - 1]
    for seed in (0, 1, 2 ** 32 + 7, 0x123456789ABCDEF, 2 ** 63 - 1):
        assert [binding.sample_key(seed, row) for row in rows] == ref.keys(seed, rows).tolist(), seed


@pytest.mark.parametrize("seed", [0, 1, 0x123456789ABCDEF])
def test_keys_are_injective(seed):
    row_keys = ref.keys(seed, np.arange(2 ** 24, dtype=np.uint32))
    assert len(np.unique(row_keys)) == 2 ** 24


def test_samples_are_nested_in_their_size():
    rng = np.random.default_rng(3)
    selected = rng.random(5_000) < 0.4
    groups = rng.integers(0, 4, size=5_000).astype(np.uint16)
    groups[rng.random(5_000) < 0.1] = ref.NO_GROUP
    for strata in (None, groups):
        smaller = ref.select(7, 0, selected, strata)
        assert not smaller.any()
        for size in (1, 2, 10, 11, 500, 501, 5_000):
            larger = ref.select(7, size, selected, strata)
            assert (larger & ~selected).sum() == 0 and (smaller & ~larger).sum() == 0, size
            if strata is None:
                assert larger.sum() == min(size, selected.sum())
            else:
                assert larger.sum() == sum(min(size, int((selected & (groups == group)).sum())) for group in range(4))
            smaller = larger
        assert np.array_equal(smaller, selected if strata is None else selected & (groups != ref.NO_GROUP))


def test_a_selection_does_not_depend_on_where_the_rows_are_cut():
    rng = np.random.default_rng(4)
    selected = rng.random(3_000) < 0.5
    tail_only = np.concatenate([np.zeros(1_000, dtype=bool), selected[1_000:]])
    whole = ref.select(9, 100, tail_only)
    assert np.array_equal(whole[1_000:], ref.select(9, 100, selected[1_000:], first_row=1_000))
    assert not np.array_equal(whole[1_000:], ref.select(9, 100, selected[1_000:], first_row=0))  # a row's number in the database matters


def test_samples_spread_over_the_row_range():
    for seed in SEEDS:
        per_tenth = np.bincount(_sample(seed) // (N_ROWS // 10), minlength=10)
        assert per_tenth.sum() == SIZE and per_tenth.min() >= 60 and per_tenth.max() <= 140, (seed, per_tenth)


def test_samples_of_two_seeds_are_independent():
    for first in SEEDS:
        for second in SEEDS:
            if first < second:
                shared = len(np.intersect1d(_sample(first), _sample(second), assume_unique=True))
                assert shared <= 40, (first, second, shared)
