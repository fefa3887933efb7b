"""The pairwise distances (K10, csrc/silo_gpu_distance.hip) through silo_gpu_distance_pack and silo_gpu_distance_pairs, against
the numpy reference of tests/pair_distances_reference.py (pinned without a GPU by tests/test_pair_distances_reference.py).

tests/test_distance_matrix_gpu.py reaches K10 through JSON and the engine.  Here the two entry points get the shapes where their
kernels take another path: positions around a word, around the chunk of words a block stages and at the length of a genome; rows
around the pair tile and at the limit of 2 048; rows of the missing symbol, of bytes outside the alphabet, identical rows and rows
that differ everywhere; the refusals of the entries.  Every comparison is an exact integer equality.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.pair_distances_reference import AA_CHARS, AA_VALID, NUC_CHARS, NUC_VALID, pack_planes, pair_distances  # noqa: E402

ALPHABETS = {"nuc": (NUC_CHARS, NUC_VALID), "aa": (AA_CHARS, AA_VALID)}
T = 16   # SILO_GPU_DISTANCE_TILE: what the row counts below stand around
C = 32   # SILO_GPU_DISTANCE_CHUNK_WORDS: what the positions below stand around
FILL = 0xA5
SENTINEL = 0xA5A5A5A5
INVALID_ARGUMENT = -1  # SILO_GPU_ERR_INVALID_ARGUMENT


def test_the_shapes_stand_around_the_kernel_constants(built):
    from silo_amd import binding

    assert (binding.DISTANCE_TILE, binding.DISTANCE_CHUNK_WORDS, binding.MAX_DISTANCE_ROWS) == (T, C, 2048)


def _draw(rng, name, n, positions, changed=0.1):
    """uint8 [n][positions]: one row of valid symbols, copied n times with a tenth of the positions redrawn from the whole
    alphabet — most positions agree."""
    all_chars, valid_chars = ALPHABETS[name]
    everything = np.frombuffer(all_chars.encode(), dtype=np.uint8)
    base = rng.choice(np.frombuffer(valid_chars.encode(), dtype=np.uint8), size=positions)
    chars = np.tile(base, (n, 1))
    redrawn = rng.random((n, positions)) < changed
    chars[redrawn] = rng.choice(everything, size=int(redrawn.sum()))
    return chars


def _pack_and_pairs(name, chars):
    """(planes as downloaded, the table) with the plane buffer and the table filled with FILL before the launches."""
    from silo_amd import binding

    n, positions = chars.shape
    planes_dev = binding.distance_pack(name, chars, fill=FILL)
    try:
        shape = (n, binding.distance_planes(name), binding.distance_words(positions))
        planes = binding.device_read(planes_dev, np.uint64, int(np.prod(shape))).reshape(shape)
        table = binding.distance_pairs(name, planes_dev, n, positions, fill=FILL)
    finally:
        binding.device_free(planes_dev)
    return planes, table


def _check_table(table, want, n):
    """Cells with i <= j equal the reference, cells with i > j still hold the sentinel, the diagonal is (0, valid count)."""
    upper = np.triu(np.ones((n, n), dtype=bool))
    assert np.array_equal(table[upper], want[upper])
    assert (table[~upper] == SENTINEL).all()
    assert not table[:, :, 0].diagonal().any() and np.array_equal(table[:, :, 1].diagonal(), want[:, :, 1].diagonal())


# ---- a: positions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("positions", [1, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1, 2 * 64 * C + 7, 29_903])
def test_positions_around_a_word_and_a_chunk(built, name, positions):
    """11 rows: the planes equal the reference's in every word — the buffer was filled with 0xA5 bytes before, so every word is
    written and the bits at or past the last position are zero — and the table equals the reference."""
    rng = np.random.default_rng(1100 + positions)
    chars = _draw(rng, name, 11, positions)
    planes, table = _pack_and_pairs(name, chars)
    assert np.array_equal(planes, pack_planes(chars, ALPHABETS[name][1]))
    want = pair_distances(chars, ALPHABETS[name][1])
    _check_table(table, want, 11)
    if positions > 1000:
        assert want[:, :, 0].max() > 20 and (want[:, :, 1] < positions).any()


# ---- b: rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
@pytest.mark.parametrize("n,positions", [(1, 130), (2, 130), (T - 1, 130), (T, 130), (T + 1, 130), (2 * T - 1, 130), (2 * T + 1, 130), (2048, 70)])
def test_rows_around_the_tile_and_at_the_limit(built, name, n, positions):
    rng = np.random.default_rng(1200 + n)
    chars = _draw(rng, name, n, positions, changed=0.2)
    _, table = _pack_and_pairs(name, chars)
    want = pair_distances(chars, ALPHABETS[name][1])
    _check_table(table, want, n)
    if n > 1:
        assert want[0, 1, 0] > 0 and want[0, -1, 1] > 0


# ---- c: special rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nuc", "aa"])
def test_special_rows(built, name):
    """Identical rows: (0, compared); a row of the missing symbol against anything: (0, 0); rows valid everywhere that differ
    everywhere: (P, P); the bytes a, ? and NUL are not valid."""
    all_chars, valid_chars = ALPHABETS[name]
    positions = 150
    rng = np.random.default_rng(1300)
    ordinary = _draw(rng, name, 1, positions, changed=0.3)[0]
    valid = np.frombuffer(valid_chars.encode(), dtype=np.uint8)
    everywhere = valid[np.arange(positions) % len(valid)]
    shifted = valid[(np.arange(positions) + 1) % len(valid)]
    strange = everywhere.copy()
    strange[[0, 64, 149]] = [ord("a"), ord("?"), 0]
    missing = np.full(positions, ord(all_chars[-1]), dtype=np.uint8)
    chars = np.stack([ordinary, ordinary, missing, everywhere, shifted, strange])
    planes, table = _pack_and_pairs(name, chars)
    assert np.array_equal(planes, pack_planes(chars, valid_chars))
    _check_table(table, pair_distances(chars, valid_chars), len(chars))
    n_valid = int(np.isin(ordinary, valid).sum())
    assert 0 < n_valid < positions and table[0, 1].tolist() == [0, n_valid]
    assert not table[2, 2:].any() and not table[:3, 2].any()
    assert table[3, 4].tolist() == [positions, positions]
    assert table[5, 5].tolist() == [0, positions - 3] and table[3, 5].tolist() == [0, positions - 3] and table[4, 5].tolist() == [positions - 3] * 2


# ---- d: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_entries(built):
    """2 049 rows, an alphabet that does not exist, NULL buffers: SILO_GPU_ERR_INVALID_ARGUMENT and nothing written; no rows or no
    positions: success and nothing written; the next valid call answers exactly."""
    from silo_amd import binding

    lib = binding.load_library()
    rng = np.random.default_rng(1400)
    chars = _draw(rng, "nuc", 3, 70)
    chars_dev = binding.device_malloc(chars.size)
    binding._check(lib.silo_gpu_memcpy_h2d(chars_dev, chars.ctypes.data_as(ctypes.c_void_p), chars.size, None))
    plane_words = 3 * 4 * 2
    planes_dev = binding.device_malloc(plane_words * 8, fill=FILL)
    table_dev = binding.device_malloc(3 * 3 * 2 * 4, fill=FILL)
    null = ctypes.c_void_p(0)

    def untouched():
        planes = binding.device_read(planes_dev, np.uint64, plane_words)
        table = binding.device_read(table_dev, np.uint32, 18)
        return (planes == 0xA5A5A5A5A5A5A5A5).all() and (table == SENTINEL).all()

    refused = [
        lib.silo_gpu_distance_pack(0, chars_dev, binding.MAX_DISTANCE_ROWS + 1, 70, planes_dev, None),
        lib.silo_gpu_distance_pairs(0, planes_dev, binding.MAX_DISTANCE_ROWS + 1, 70, table_dev, None),
        lib.silo_gpu_distance_pack(2, chars_dev, 3, 70, planes_dev, None),
        lib.silo_gpu_distance_pairs(-1, planes_dev, 3, 70, table_dev, None),
        lib.silo_gpu_distance_pack(0, null, 3, 70, planes_dev, None),
        lib.silo_gpu_distance_pack(0, chars_dev, 3, 70, null, None),
        lib.silo_gpu_distance_pairs(1, null, 3, 70, table_dev, None),
        lib.silo_gpu_distance_pairs(1, planes_dev, 3, 70, null, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused)
    assert b"silo_gpu_distance_pairs" in lib.silo_gpu_last_error()
    succeeded = [
        lib.silo_gpu_distance_pack(0, chars_dev, 0, 70, planes_dev, None),
        lib.silo_gpu_distance_pack(0, chars_dev, 3, 0, planes_dev, None),
        lib.silo_gpu_distance_pairs(0, planes_dev, 0, 70, table_dev, None),
        lib.silo_gpu_distance_pairs(0, planes_dev, 3, 0, table_dev, None),
    ]
    assert succeeded == [0] * len(succeeded)
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert untouched()
    # the valid call on the same buffers
    binding._check(lib.silo_gpu_distance_pack(0, chars_dev, 3, 70, planes_dev, None))
    binding._check(lib.silo_gpu_distance_pairs(0, planes_dev, 3, 70, table_dev, None))
    binding._check(lib.silo_gpu_stream_synchronize(None))
    assert np.array_equal(binding.device_read(planes_dev, np.uint64, plane_words).reshape(3, 4, 2), pack_planes(chars, NUC_VALID))
    _check_table(binding.device_read(table_dev, np.uint32, 18).reshape(3, 3, 2), pair_distances(chars, NUC_VALID), 3)
    for pointer in (chars_dev, planes_dev, table_dev):
        binding.device_free(pointer)
