"""silo_gpu_smallest_keys (K21, csrc/silo_gpu_distinct_counts.hip) alone: the k smallest of n pairwise distinct 64-bit keys whose
number the device alone knows, against np.sort — list lengths around a block of 256 and 70 001, in a list with room behind n whose
0xA5 keys must not be read as keys; k from 1 to past n and the largest there is; keys that are random, that differ in their lowest
or their highest byte only, that are class keys with many equal counts, ascending and descending.  Every comparison is an exact
equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILLED = np.uint64(0xA5A5A5A5A5A5A5A5)
LENGTHS = [0, 1, 255, 256, 257, 70_001]
KINDS = ["random", "low byte", "high byte", "class keys", "ascending", "descending"]
GUARD_WORDS = 2
ROOM = 77  # keys behind n
CASES = [(n, kind) for n in LENGTHS for kind in KINDS if n <= 256 or kind not in ("low byte", "high byte")]  # (256 values of a byte)


@functools.lru_cache(maxsize=None)
def key_list(kind, n):
    """uint64 [n], pairwise distinct."""
    rng = np.random.default_rng(2100 + n + 13 * KINDS.index(kind))
    if kind in ("low byte", "high byte"):
        digits = rng.permutation(256)[:n].astype(np.uint64)
        keys = np.uint64(0x0123456789ABCD00) | digits if kind == "low byte" else np.uint64(0x00A5A5A5A5A5A5A5) | (digits << np.uint64(56))
    elif kind == "class keys":  # (~count << 32) | row: a few large classes, many equal small counts
        rows = rng.permutation(max(n * 3, 1))[:n].astype(np.uint64)
        counts = np.where(rng.random(n) < 0.05, rng.integers(2, 5000, size=n), rng.integers(1, 4, size=n)).astype(np.uint64)
        keys = ((np.uint64(0xFFFFFFFF) - counts) << np.uint64(32)) | rows
    else:
        keys = np.unique(rng.integers(0, 1 << 63, size=2 * n + 8, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=2 * n + 8, dtype=np.uint64))
        keys = rng.permutation(keys)[:n]
        if kind == "ascending":
            keys = np.sort(keys)
        if kind == "descending":
            keys = np.sort(keys)[::-1].copy()
    assert len(keys) == n == len(np.unique(keys))
    keys.setflags(write=False)
    return keys


def _select(keys, k, calls=1):
    from silo_amd import binding

    n = len(keys)
    listed = np.full(n + ROOM, FILLED, dtype=np.uint64)
    listed[:n] = keys
    out, count = binding.smallest_keys(listed, n, k, fill=FILL, guard_words=GUARD_WORDS, calls=calls)
    assert count == min(n, k)
    assert (out[count:] == FILLED).all()
    return np.sort(out[:count])


@pytest.mark.parametrize("n,kind", CASES)
def test_the_smallest_keys_match_numpy(built, n, kind):
    from silo_amd import binding

    keys = key_list(kind, n)
    ordered = np.sort(keys)
    for k in sorted({1, n - 1, n, n + 1, binding.MAX_DISTINCT_CLASSES}):
        if not 1 <= k <= binding.MAX_DISTINCT_CLASSES:
            continue
        got = _select(keys, k, calls=2 if k == 1 else 1)
        assert np.array_equal(got, ordered[:k]), k
    if kind == "class keys" and n == 70_001:
        counts = np.uint64(0xFFFFFFFF) - (keys >> np.uint64(32))
        assert len(np.unique(counts)) < n // 10 and counts.max() > 1000  # many equal counts: the rounds are decided in the low word


def test_a_list_that_is_longer_than_its_room(built):
    """*n_keys_dev above the capacity: the keys of the list are the first `capacity`."""
    from silo_amd import binding

    keys = key_list("random", 257)
    out, count = binding.smallest_keys(keys, 70_001, 300, fill=FILL, guard_words=GUARD_WORDS)
    assert count == 257 and np.array_equal(np.sort(out[:257]), np.sort(keys)) and (out[257:] == FILLED).all()
    out, count = binding.smallest_keys(keys, 70_001, 5, fill=FILL, guard_words=GUARD_WORDS)
    assert count == 5 and np.array_equal(np.sort(out[:5]), np.sort(keys)[:5]) and (out[5:] == FILLED).all()


def test_refusals_write_nothing(built):
    from silo_amd import binding

    lib = binding.load_library()
    capacity, k = 64, 8
    keys = binding._upload(np.arange(capacity, dtype=np.uint64))
    n_keys = binding._upload(np.array([capacity], dtype=np.uint32))
    out = binding.device_malloc(k * 8, FILL)
    out_count = binding.device_malloc(4, FILL)
    scratch = binding.device_malloc(binding.SMALLEST_KEYS_SCRATCH_BYTES, FILL)
    try:
        for arguments in ((None, n_keys, capacity, k, out, out_count, scratch), (keys, None, capacity, k, out, out_count, scratch),
                          (keys, n_keys, capacity, k, None, out_count, scratch), (keys, n_keys, capacity, k, out, None, scratch),
                          (keys, n_keys, capacity, k, out, out_count, None), (keys, n_keys, 0, k, out, out_count, scratch),
                          (keys, n_keys, capacity, 0, out, out_count, scratch),
                          (keys, n_keys, capacity, binding.MAX_DISTINCT_CLASSES + 1, out, out_count, scratch)):
            assert lib.silo_gpu_smallest_keys(*arguments, None) != 0, arguments
        binding._check(lib.silo_gpu_stream_synchronize(None))
        assert (binding.device_read(out, np.uint64, k) == FILLED).all()
        assert (binding.device_read(out_count, np.uint32, 1) == 0xA5A5A5A5).all()
        assert (binding.device_read(scratch, np.uint8, binding.SMALLEST_KEYS_SCRATCH_BYTES) == FILL).all()
        # ... and a call that is in order is taken
        binding._check(lib.silo_gpu_smallest_keys(keys, n_keys, capacity, k, out, out_count, scratch, None))
        binding._check(lib.silo_gpu_stream_synchronize(None))
        assert np.array_equal(np.sort(binding.device_read(out, np.uint64, k)), np.arange(k, dtype=np.uint64))
        assert binding.device_read(out_count, np.uint32, 1)[0] == k
    finally:
        for ptr in (keys, n_keys, out, out_count, scratch):
            binding.device_free(ptr)
