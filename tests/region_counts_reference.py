"""The numpy statement of K23 (CellCount over a position range / CellCountByRegion): per row of a symbol matrix and per region
[first, end) of positions the number of cells whose class is one of the kinds of a mask, the rows a pair of bounds selects, the
per-region counts of a selection and the host colouring of overlapping regions into chunks of disjoint ones.

Built on tests/cell_counts_reference.py: the value of a region is the whole-sequence value of the column slice sym[:, first:end]
against reference[first:end] — `cells` decides the class of a cell, nothing here does."""
import numpy as np

from tests import cell_counts_reference as whole

MAX_REGIONS = 256
REGION_VALUE_BUDGET_BYTES = 256 << 20


def region_cells(sym, reference, alphabet, ranges):
    """uint32 [len(ranges)][rows][4]: the four cell counts of every row inside each region (they do not depend on a mask)."""
    sym = np.asarray(sym)
    reference = np.asarray(reference)
    return np.stack([whole.cells(sym[:, first:end], reference[first:end], alphabet) for first, end in ranges])


def values_of_cells(cells, kinds_mask):
    """uint32 [len(ranges)][rows] from region_cells' result."""
    return np.stack([whole.values(table, kinds_mask) for table in cells]).astype(np.uint32)


def values(sym, reference, alphabet, ranges, kinds_mask):
    """uint32 [len(ranges)][rows]: value(r, g), ranges 0-based and half-open."""
    return values_of_cells(region_cells(sym, reference, alphabet, ranges), kinds_mask)


def selected(column, n, at_least=0, at_most=0xFFFFFFFF):
    """bool [rows of the column]: row < n and at_least <= value <= at_most."""
    column = np.asarray(column, dtype=np.uint64)
    return (np.arange(len(column)) < n) & (column >= np.uint64(at_least)) & (column <= np.uint64(at_most))


def counts(columns, rows, bounds):
    """uint64 [len(columns)]: per column the rows of `rows` (bool over the columns' rows) with bounds[c][0] <= value <= bounds[c][1]."""
    rows = np.asarray(rows, dtype=bool)
    return np.array([int((selected(column, len(column), low, high) & rows).sum()) for column, (low, high) in zip(columns, bounds)], dtype=np.uint64)


def bitset_words(bits, row_words):
    """uint64 [row_words]: bool rows as the words of a device bitset (bit i of word w = row 64 w + i)."""
    padded = np.zeros(row_words * 64, dtype=np.uint8)
    padded[:len(bits)] = np.asarray(bits, dtype=np.uint8)
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64)


def colour(ranges, max_regions=MAX_REGIONS):
    """The chunks of CellCountByRegion: lists of indices into `ranges`.  Sorted by start (ties in request order), each region goes
    into the first chunk in which it overlaps none and which has fewer than max_regions regions."""
    chunks = []
    for region in sorted(range(len(ranges)), key=lambda g: ranges[g][0]):
        for chunk in chunks:
            if len(chunk) < max_regions and ranges[chunk[-1]][1] <= ranges[region][0]:
                chunk.append(region)
                break
        else:
            chunks.append([region])
    return chunks


def chunk_regions(row_words, budget_bytes=REGION_VALUE_BUDGET_BYTES):
    """The most regions a chunk may hold for a largest partition of `row_words` row words: at least one, at most MAX_REGIONS."""
    return max(1, min(MAX_REGIONS, budget_bytes // (row_words * 64 * 4)))


def response_rows(names, ranges, counted, total):
    """The rows of a CellCountByRegion response in request order."""
    return [{"region": name, "positionFrom": first + 1, "positionTo": end, "count": int(count), "total": int(total)}
            for name, (first, end), count in zip(names, ranges, counted)]
