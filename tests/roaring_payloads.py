"""Roaring payloads for the import tests, written with numpy — test infrastructure only.

serialize_ids writes the portable format exactly as oracle/roaring_format.py does (same container choice, same bytes; pinned by
tests/test_roaring_payloads_reference.py), but a container at a time instead of a value at a time: the matrix of
tests/test_roaring_import_shapes_gpu.py needs some thousand payloads of stores with up to 140 001 rows.  The module also holds the
columns of that matrix (import_cases), so that the CPU test can take the census of the container kinds the GPU test will meet.
"""
import functools
import struct
from dataclasses import dataclass
from typing import Optional

import numpy as np

SERIAL_COOKIE_NO_RUNCONTAINER = 12346
SERIAL_COOKIE = 12347
NO_OFFSET_THRESHOLD = 4
EMPTY = struct.pack("<II", SERIAL_COOKIE_NO_RUNCONTAINER, 0)  # the bitmap without a container

NUC_CHARS = np.frombuffer(b"-ACGTRYSWKMBDHVN", dtype=np.uint8)
AA_CHARS = np.frombuffer(b"-ACDEFGHIKLMNPQRSTVWYBZ*X", dtype=np.uint8)


def serialize_ids(ids, use_runs):
    """ids: integers in [0, 2**32), any order, duplicates allowed -> the bytes oracle.roaring_format.serialize gives for them."""
    ids = np.asarray(ids, dtype=np.int64).ravel()
    if len(ids) > 1 and not (ids[1:] > ids[:-1]).all():
        ids = np.unique(ids)
    keys = ids >> 16
    low = (ids & 0xFFFF).astype("<u2")
    first = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0] if len(ids) else np.zeros(0, dtype=np.int64)
    ends = np.r_[first[1:], len(ids)]
    containers = []  # (key, cardinality, is_run, data)
    for begin, end in zip(first.tolist(), ends.tolist()):
        values = low[begin:end]
        cardinality = end - begin
        plain_size = 2 * cardinality if cardinality <= 4096 else 8192
        wide = values.astype(np.int64)
        starts = np.nonzero(np.r_[True, wide[1:] != wide[:-1] + 1])[0]
        if use_runs and 2 + 4 * len(starts) < plain_size:
            runs = np.empty((len(starts), 2), dtype="<u2")
            runs[:, 0] = values[starts]
            runs[:, 1] = wide[np.r_[starts[1:], cardinality] - 1] - wide[starts]
            data = struct.pack("<H", len(starts)) + runs.tobytes()
            is_run = True
        elif cardinality <= 4096:
            data, is_run = values.tobytes(), False
        else:
            bits = np.zeros(65536, dtype=bool)
            bits[wide] = True
            data, is_run = np.packbits(bits, bitorder="little").tobytes(), False  # = 1024 little-endian uint64 words
        containers.append((int(keys[begin]), cardinality, is_run, data))
    n = len(containers)
    any_run = any(is_run for _, _, is_run, _ in containers)
    if any_run:
        flags = bytearray((n + 7) // 8)
        for k, (_, _, is_run, _) in enumerate(containers):
            if is_run:
                flags[k // 8] |= 1 << (k % 8)
        header = struct.pack("<I", SERIAL_COOKIE | ((n - 1) << 16)) + bytes(flags)
    else:
        header = struct.pack("<II", SERIAL_COOKIE_NO_RUNCONTAINER, n)
    header += b"".join(struct.pack("<HH", key, cardinality - 1) for key, cardinality, _, _ in containers)
    offsets = b""
    if not any_run or n >= NO_OFFSET_THRESHOLD:
        offset = len(header) + 4 * n
        for _, _, _, data in containers:
            offsets += struct.pack("<I", offset)
            offset += len(data)
    return header + offsets + b"".join(data for _, _, _, data in containers)


def container_directory(payload):
    """[(kind, cardinality)] per container — kind 'array' | 'bitset' | 'run' — from the directory alone (cookie, run flags,
    cardinalities)."""
    if len(payload) == 0:
        return []
    (cookie,) = struct.unpack_from("<I", payload, 0)
    cursor = 4
    flags = None
    if cookie & 0xFFFF == SERIAL_COOKIE:
        n = (cookie >> 16) + 1
        flags = payload[cursor:cursor + (n + 7) // 8]
        cursor += (n + 7) // 8
    elif cookie == SERIAL_COOKIE_NO_RUNCONTAINER:
        (n,) = struct.unpack_from("<I", payload, cursor)
        cursor += 4
    else:
        raise ValueError("unknown cookie")
    directory = []
    for k in range(n):
        cardinality = struct.unpack_from("<H", payload, cursor + 4 * k + 2)[0] + 1
        if flags is not None and (flags[k // 8] >> (k % 8)) & 1:
            directory.append(("run", cardinality))
        else:
            directory.append(("array" if cardinality <= 4096 else "bitset", cardinality))
    return directory


def container_kinds(payload):
    """'array' | 'bitset' | 'run' per container."""
    return [kind for kind, _ in container_directory(payload)]


STATES = ("plain", "flipped", "flipped_max", "deleted")


def most_numerous_symbol(column, n_symbols, missing, reference_symbol):
    """The non-missing symbol with the most rows, the lowest id among equals — the reference symbol where no row has one."""
    counts = np.bincount(column, minlength=n_symbols)[:n_symbols].copy()
    counts[missing] = 0
    return int(np.argmax(counts)) if counts.any() else int(reference_symbol)


def position_payloads(column, n_symbols, missing, state, use_runs, reference_symbol):
    """One column of symbol ids as the reference would hold the Position -> ({symbol: payload}, flipped, deleted).
    plain: every non-empty bitmap as it is.  flipped: the reference symbol's bitmap is its complement over [0, n) — present even
    when empty.  flipped_max: the same for the most numerous non-missing symbol.  deleted: that symbol has no payload and is named
    as deleted.  The missing symbol never has a payload (it is stored row-wise: missing_row_payloads)."""
    assert state in STATES
    column = np.asarray(column)
    special = None
    if state == "flipped":
        special = int(reference_symbol)
    elif state in ("flipped_max", "deleted"):
        special = most_numerous_symbol(column, n_symbols, missing, reference_symbol)
    payloads = {}
    for symbol in range(n_symbols):
        if symbol == missing or (state == "deleted" and symbol == special):
            continue
        flipped = state in ("flipped", "flipped_max") and symbol == special
        ids = np.nonzero((column != symbol) if flipped else (column == symbol))[0]
        if len(ids) or flipped:
            payloads[symbol] = serialize_ids(ids, use_runs)
    return payloads, (special if state in ("flipped", "flipped_max") else None), (special if state == "deleted" else None)


def missing_row_payloads(sym, missing, use_runs):
    """Per row of the symbol matrix the bitmap of the positions where it holds the missing symbol; rows without one alternate
    between no bytes at all and the empty bitmap."""
    is_missing = np.asarray(sym) == missing
    out = [b"" if row % 2 == 0 else EMPTY for row in range(len(is_missing))]
    for row in np.nonzero(is_missing.any(axis=1))[0].tolist():
        out[row] = serialize_ids(np.nonzero(is_missing[row])[0], use_runs)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_roaring_import_shapes_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------
POSITIONS = 8
P4_EVEN_END = 8192   # symbol 1 at the even ids below: 4 096 rows, the largest array container
P4_ODD_END = 8194    # symbol 2 at the odd ids below: 4 097 rows, the smallest bitset container
P5_HEAD_ROWS = 128   # position 5: the missing symbol in these first rows ...
P5_TAIL_ROWS = 65    # ... and in these last ones (the ragged tail word and the word before it)


@dataclass(frozen=True)
class ImportCase:
    name: str
    n: int
    alphabet: str                 # 'nuc' | 'aa'
    sym: np.ndarray               # uint8 [n][POSITIONS] symbol ids; a null genome holds the missing symbol everywhere
    is_null: np.ndarray           # uint8 [n]
    reference: np.ndarray         # uint8 [POSITIONS]: a valid symbol per position
    extra_symbols: Optional[tuple]  # symbols that get a column plane of their own (None: the missing symbol alone)

    @property
    def n_symbols(self):
        return 16 if self.alphabet == "nuc" else 25

    @property
    def missing(self):
        return 15 if self.alphabet == "nuc" else 24

    @property
    def ambiguity(self):
        return 5 if self.alphabet == "nuc" else 21  # R / B: neither a valid mutation symbol nor the missing one

    @property
    def chars(self):
        return NUC_CHARS if self.alphabet == "nuc" else AA_CHARS

    def boundary_rows(self):
        return np.array(sorted({r for r in (0, 63, 64, 65535, 65536, self.n - 1) if 0 <= r < self.n}), dtype=np.int64)

    def store_description(self):
        description = dict(name="s", alphabet=self.alphabet, reference=self.reference.copy())
        if self.extra_symbols is not None:
            description["extra_symbols"] = list(self.extra_symbols)
        return description


REFERENCE = np.array([1, 2, 1, 1, 4, 1, 2, 1], dtype=np.uint8)  # ids 1..4 are valid mutation symbols of both alphabets


def _columns(n, alphabet, seed, all_missing_5=False):
    """The eight columns (see import_case), then the missing symbol laid over them."""
    rng = np.random.default_rng(seed)
    n_symbols = 16 if alphabet == "nuc" else 25
    missing = n_symbols - 1
    valid = np.array([0, 1, 2, 3, 4] if alphabet == "nuc" else list(range(21)) + [23])
    rows = np.arange(n)
    sym = np.empty((n, POSITIONS), dtype=np.uint8)
    # 0: the reference symbol in 99.8 % of the rows, the rest spread over the other valid symbols
    others = valid[valid != REFERENCE[0]]
    sym[:, 0] = np.where(rng.random(n) < 0.998, REFERENCE[0], others[rng.integers(0, len(others), size=n)])
    # 1: uniform over every symbol but the missing one
    sym[:, 1] = rng.integers(0, n_symbols - 1, size=n)
    # 2: five blocks of one symbol each; one of them is the single row 65 536, the first of the second container
    edges = np.minimum(np.array([0, 30000, 65536, 65537, 120000, n]), n)
    for block, symbol in enumerate((1, 2, 3, 4, 0)):
        sym[edges[block]:edges[block + 1], 2] = symbol
    # 3: one valid symbol everywhere, not the reference symbol
    sym[:, 3] = 3
    # 4 (written below, after the missing symbol): 4 096 even ids, 4 097 odd ids, a third symbol everywhere else
    sym[:, 4] = 4
    # 5: the reference symbol nowhere; the missing symbol at both ends, one other valid symbol between them
    sym[:, 5] = 2
    # 6: 90 % one symbol, the rest uniform over the valid symbols; an ambiguity code at the container and word boundaries
    sym[:, 6] = np.where(rng.random(n) < 0.9, 2, valid[rng.integers(0, len(valid), size=n)])
    # 7: two symbols, half of the rows each; the reference symbol has no row
    sym[:, 7] = np.where(rng.random(n) < 0.5, 3, 4)
    # the missing symbol: 1 % of the rows carry one run of it over 2-5 positions, 0.25 % are null genomes (drawn past the rows
    # that position 4 counts, where the store has such rows)
    run_rows = np.nonzero(rng.random(n) < 0.01)[0]
    starts = rng.integers(0, POSITIONS - 1, size=len(run_rows))
    lengths = rng.integers(2, 6, size=len(run_rows))
    for row, start, length in zip(run_rows.tolist(), starts.tolist(), lengths.tolist()):
        sym[row, start:min(POSITIONS, start + length)] = missing
    is_null = (rng.random(n) < 0.0025) & ((rows >= P4_ODD_END) | (n <= P4_ODD_END))
    sym[(rows < P5_HEAD_ROWS) | (rows >= n - P5_TAIL_ROWS) | all_missing_5, 5] = missing
    head = rows < P4_ODD_END
    sym[head & (rows % 2 == 0) & (rows < P4_EVEN_END) & ~is_null, 4] = 1
    sym[head & (rows % 2 == 1) & ~is_null, 4] = 2
    sym[head & (rows % 2 == 0) & (rows >= P4_EVEN_END) & ~is_null, 4] = 4
    ambiguity = 5 if alphabet == "nuc" else 21
    for row in (0, 63, 64, 65535, 65536, n - 1):
        if 0 <= row < n:
            sym[row, 6] = ambiguity
    sym[is_null] = missing
    return sym, is_null.astype(np.uint8)


SIZES = ((1, "nuc"), (64, "nuc"), (65537, "aa"), (140001, "nuc"))
SMALLEST, LARGEST = "n1-nuc", "n140001-nuc"
EXTRA_PLANE = "n140001-nuc-extra"
ALL_MISSING = "n65537-aa-allmissing"
VARIANTS = {EXTRA_PLANE: "n140001-nuc", ALL_MISSING: ALL_MISSING}  # variant -> the case whose payloads it imports


@functools.lru_cache(maxsize=None)
def import_case(name):
    """Stores of one sequence store with 8 positions; seeded, the same arrays on every call (treat them as read-only).

    n = 1 (one row), 64 (exactly one word), 65 537 amino acids (the second container holds one row, in a 1-bit tail word),
    140 001 (three containers, n % 64 == 33); n140001-nuc-extra holds the columns of n140001-nuc in a store created with
    extra_symbols = [missing, R], so that the ambiguity code of position 6 lives in a column plane of its own; in
    n65537-aa-allmissing EVERY row of position 5 holds the missing symbol (else the columns of n65537-aa): no payload at all
    there and a deleted reference symbol without a row, past row 65 535 and over the 1-bit tail word — a store that keeps the
    plane of the missing symbol and derives nothing.

    Columns (symbol ids; 1..4 are A C G T / A C D E): 0 the reference symbol in 99.8 % of the rows; 1 uniform over all symbols
    but the missing one; 2 five blocks with edges 0, 30 000, 65 536, 65 537, 120 000, n; 3 one symbol everywhere; 4 symbol 1 at the
    even ids 0..8190, symbol 2 at the odd ids 1..8193, symbol 4 elsewhere (rows below 8 194 never miss it); 5 the missing symbol in
    the first 128 and the last 65 rows — every row of the two small stores, which then have no payload at all there and a deleted
    reference symbol without a row — and one symbol between; 6 one symbol in 90 % with an ambiguity code at rows 0, 63, 64, 65 535,
    65 536, n - 1; 7 two symbols at 50 %, neither the reference symbol.  1 % of the rows carry one run of the missing symbol over
    2-5 positions, 0.25 % are null genomes.

    The missing symbol is rationed (no column that is missing in every row of a large store, none in column 1): finalize keeps
    the missing symbol as runs only where they take less than a quarter of its planes, which for 8 positions is one run in 2 % of
    the rows, and only such a store derives a symbol — the mixed layouts the GPU test asserts at n >= 65 537."""
    for n, alphabet in SIZES:
        if name in (f"n{n}-{alphabet}", f"n{n}-{alphabet}-extra", f"n{n}-{alphabet}-allmissing"):
            sym, is_null = _columns(n, alphabet, seed=1000 + n, all_missing_5=name.endswith("-allmissing"))
            sym.setflags(write=False)
            is_null.setflags(write=False)
            extra = None
            if name.endswith("-extra"):
                extra = (15, 5) if alphabet == "nuc" else (24, 21)
            return ImportCase(name, n, alphabet, sym, is_null, REFERENCE.copy(), extra)
    raise KeyError(name)


def case_names():
    return [f"n{n}-{alphabet}" for n, alphabet in SIZES]


def case_payloads(name, state, use_runs):
    """[({symbol: payload}, flipped, deleted) per position] of a case; cached, the GPU test asks once per layout."""
    return _case_payloads(VARIANTS.get(name, name), state, use_runs)


@functools.lru_cache(maxsize=None)
def _case_payloads(name, state, use_runs):
    case = import_case(name)
    return tuple(
        position_payloads(case.sym[:, p], case.n_symbols, case.missing, state, use_runs, int(case.reference[p])) for p in range(POSITIONS)
    )


def case_missing_rows(name, use_runs):
    return _case_missing_rows(VARIANTS.get(name, name), use_runs)


@functools.lru_cache(maxsize=None)
def _case_missing_rows(name, use_runs):
    case = import_case(name)
    return tuple(missing_row_payloads(case.sym, case.missing, use_runs))
