// scan_internal.h — what the translation units of the Mutations scan (K1) share beside store_internal.h: the
// by-value argument structs of their kernels, the pieces a scan is cut into, and the one host function each pass exports.
//   silo_gpu_scan.hip          the scan over ranges: pieces, timing log, scratch pool, side streams, the C entries
//   silo_gpu_scan_planes.hip   the plane rows: k_scan_sliced, k_scan_sliced_rowwave, k_compact_filter (prepare), k_scan_gather
//   silo_gpu_scan_keys.hip     the escape keys, the gap events, the end events: k_scan_escapes_sliced, k_scan_escapes, k_scan_escapes_overflow
//   silo_gpu_scan_derived.hip  derived symbols: k_scan_missing_runs, k_sum_run_parts, k_count_sparse_keys, k_finish_scan
// A kernel lives in the anonymous namespace of its file and is launched only from there.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <vector>

#include "store_internal.h"

namespace silo_gpu_detail {

constexpr uint32_t SCAN_MAX_RANGES = 32;
// the per-filter sector counters sit 256 bytes apart: atomics on one L2 channel serialise (~12 ns each), and a dense
// filter makes every block add to its counter
constexpr uint32_t SPARSE_COUNTER_STRIDE = 64;
constexpr uint32_t SECTOR_WORDS = 8;        // a 64-byte sector of a filter row
constexpr uint32_t COMPACT_THREADS = 1024;   // words per block of k_compact_filter
// rows of a run of one-hot rows whose live rows a block of k_scan_sliced can list in LDS (4 KiB); a run of more rows is scanned in full
constexpr uint32_t ROW_LIST_MAX = 1024;

/// Which scan serves a filter, from the counters k_compact_filter left for it: [0] sectors with a set bit, [1] stretches of
/// COMPACT_THREADS words with one.  The gather pays while the sectors fit its list AND cost less than the column tiles the
/// dense scan cannot skip: it reads its sectors at about 0.6 of the dense scan's rate, so a clustered filter (rows in
/// lineage or date order: few sectors because they are contiguous, not because they are few) stays with the dense scan.
__device__ __forceinline__ bool takesGatherScan(const uint32_t* __restrict__ counters, uint32_t capacity) {
   const uint32_t sectors = counters[0];
   return sectors <= capacity && static_cast<uint64_t>(sectors) * 8u < static_cast<uint64_t>(counters[1]) * (COMPACT_THREADS / SECTOR_WORDS) * 5u;
}

/// One launch of the scan: up to SILO_GPU_MAX_SCAN_BATCH filters against up to SCAN_MAX_RANGES position ranges of
/// sequence stores with the same layout (the 12 genes of an AminoAcidMutations query, the segments of a segmented
/// genome): blocks (k_scan_sliced) or waves (k_scan_gather) are dealt to the ranges by first_unit.
struct ScanBatchArgs {
   const uint64_t* filters[SILO_GPU_MAX_SCAN_BATCH];
   // sparse-filter routing (K1s): sparse_sectors[q * SPARSE_COUNTER_STRIDE] = number of 64-byte sectors of filter q with a set bit, written by
   // k_compact_filter earlier on the same stream; a filter with at most sparse_capacity of them is served by
   // k_scan_gather and is treated as empty by k_scan_sliced.  nullptr = no routing.
   const uint32_t* sparse_sectors;
   uint32_t sparse_capacity;
   uint32_t n_ranges;
   const uint64_t* planes[SCAN_MAX_RANGES];    // first plane row of the range
   uint32_t n_positions[SCAN_MAX_RANGES];
   uint32_t first_unit[SCAN_MAX_RANGES + 1];   // prefix sums of the blocks / waves per range
   uint32_t* counts[SCAN_MAX_RANGES][SILO_GPU_MAX_SCAN_BATCH];  // counts[range][filter], at the first position of the range
   // mapped layouts (2 or 3 code planes): per position of the range CODE_MAP_STRIDE bytes, [c] = the scan symbol that
   // code c stands for at this position (0xFF = none); out_symbols = symbols per position of the count tables (5 / 22)
   // one-hot rows (KIND_ROWS): the range is a run of plane ROWS, n_positions counts rows, code_map[range] points at the
   // uint32 table row -> position * out_symbols + symbol (positions of the store), target_base = that of counts[range]
   const uint8_t* code_map[SCAN_MAX_RANGES];
   uint32_t target_base[SCAN_MAX_RANGES];
   uint32_t out_symbols;
   // one-hot rows of a range that counts the gap symbol's end runs (DerivedPlan::end_runs): one byte per row from the range's first
   // row on (SeqStoreHost::Layout::d_row_covered), non-zero = the row is not read, by k_scan_sliced and k_scan_gather alike; else nullptr
   const uint8_t* row_covered[SCAN_MAX_RANGES];
};

// what a run of plane rows holds
enum : int { KIND_IDENTITY = 0, KIND_MAPPED = 1, KIND_ROWS = 2 };

/// What a launch over one-hot rows (KIND_ROWS) needs to leave out the rows no Mutations row can come from
/// (silo_gpu_mutations_scan_ranges_min_proportion), as the escape pass leaves out granules of keys (EscapeSliceArgs): the counters
/// of the prepare step ([q * SPARSE_COUNTER_STRIDE + 2] = the cardinality of filter q of the launch), every filter's proportion,
/// and per range the two bounds of its rows (SeqStoreHost::Layout::d_row_heaviest, d_row_without, from the range's first row on).
/// A range with null bounds — every range of an exact scan, and of the other kinds of launch — walks all its rows.
struct RowPruneArgs {
   const uint32_t* counters;
   double min_proportion[SILO_GPU_MAX_SCAN_BATCH];
   const uint32_t* heaviest[SCAN_MAX_RANGES];
   const uint32_t* without[SCAN_MAX_RANGES];
};
static_assert(sizeof(ScanBatchArgs) + sizeof(RowPruneArgs) + 3 * sizeof(uint32_t) <= 4096, "k_scan_sliced takes its arguments by value: the kernel-argument segment holds 4 KiB");

/// The filter pointers of a launch (every by-value argument struct begins with them).
inline void copyFilters(const uint64_t* (&dst)[SILO_GPU_MAX_SCAN_BATCH], const uint64_t* const* filters, uint32_t n) {
   std::copy_n(filters, n, dst);
}

/// The part of a range that lies in ONE run of its store's layout: what a launch takes.
struct ScanPiece {
   const uint64_t* planes;    // first plane row of the piece
   const uint8_t* code_map;   // of the piece's first position (mapped layouts); the row targets of its first row (one-hot rows); else nullptr
   uint32_t n_positions;      // one-hot rows: plane rows
   uint32_t target_base;      // one-hot rows: first position of the piece * n_scan
   const uint32_t* row_heaviest;  // one-hot rows: the bounds of the piece's rows from its first row on (RowPruneArgs), or nullptr
   const uint32_t* row_without;
   const uint8_t* row_covered;    // one-hot rows of a range that counts end runs: the flags of the piece's rows from its first row on, or nullptr
   uint32_t* counts[SILO_GPU_MAX_SCAN_BATCH];  // tables at the piece's first position
};

/// The four plane layouts the scan kernels are instantiated for.
enum ScanLayout { SCAN_2_PLANES = 0, SCAN_3_PLANES_MAPPED, SCAN_FULL_NUCLEOTIDE, SCAN_FULL_AMINO_ACID, SCAN_ONE_HOT_ROWS, N_SCAN_LAYOUTS };

// Derived symbols (silo_gpu_scan_derived.hip): the scan over ranges owns the plan, the passes fill and read it.
constexpr uint32_t DERIVED_MAX_RANGES = 16;

/// A range of a scan with derived symbols.  Its private tables: per filter `stride` words of scratch — counts[n][n_scan], then
/// diff[n + 1] (selected rows entering / leaving a run of the missing symbol at each position), then ambiguous[n]; with gap events
/// gaps[n][2] instead of the two, and behind it, in a range that counts end runs (position_covered != nullptr), ends[n][2]: the
/// selected rows whose leading run of the gap symbol ends ([0]) and whose trailing run begins ([1]) at each position.
struct DerivedRange {
   uint32_t* scratch;        // of filter 0
   uint32_t stride;          // words per filter
   uint32_t n_positions;
   uint32_t n_scan;
   uint32_t pos_begin;
   uint32_t gaps_offset;     // words from a filter's counts to its gaps (its diff): n_positions * n_scan rounded up to 16 bytes
   uint32_t ends_offset;     // words from a filter's counts to its ends, rounded up likewise (a range that counts end runs)
   uint32_t table_offset;    // a scan that selects (SelectSink): the range's first position in the filters' count tables
   const uint8_t* code_map;  // of the store's position 0; nullptr: no position of this store derives a symbol
   const uint8_t* position_covered;  // of the store's position 0: the gap symbol's cell takes its end runs from ends[n][2]; nullptr: no end runs
   uint32_t end_symbol;              // the gap symbol's scan index
   const uint64_t* run_keys;
   const uint32_t* run_ends;
   const uint32_t* run_slice_first;  // [n_run_slices + 1]
   const uint64_t* sparse_keys;      // position << 37 | symbol << 32 | sequence, ascending
   uint32_t sparse_begin;            // the keys of the range's positions
   uint32_t sparse_end;
   uint32_t* caller_counts[SILO_GPU_MAX_SCAN_BATCH];  // at the range's first position
};
/// Where k_finish_scan delivers the Mutations rows of one filter of a scan that selects (silo_gpu_mutations_scan_select): the
/// filter's row slot (silo_gpu_row_slot: cursor and ticket on the device, rows and header word in page-locked host memory), what
/// the selection needs beside the counts, and how many blocks of the scan's finish launches take a ticket for this filter.
struct SelectSink {
   const uint8_t* reference_index;  // of the table's position 0
   uint32_t* cursor_and_ticket;
   silo_gpu_mutation_row* host_rows;
   unsigned long long* host_header;
   double min_proportion;
   uint32_t capacity;
   uint32_t epoch;
   uint32_t total_blocks;
};
struct DerivedArgs {
   const uint64_t* filters[SILO_GPU_MAX_SCAN_BATCH];
   const uint32_t* counters;  // of the prepare step: [q * SPARSE_COUNTER_STRIDE + 2] = the cardinality of filter q
   uint32_t row_words;
   uint32_t n_run_slices;
   uint32_t n_ranges;
   uint32_t first_unit[DERIVED_MAX_RANGES + 1];  // blocks per range (k_count_sparse_keys, k_finish_scan: each their own)
   // k_scan_missing_runs with the diff in LDS: a block hands its diff over as a part — [filter][range][slice][block of the slice]
   // x part_stride words, plain stores — and raises its flag (zeroed by the prepare step); k_sum_run_parts adds the parts up
   uint32_t* run_parts;
   uint32_t* run_flags;
   uint32_t part_stride;
   uint32_t run_blocks_per_slice;
   DerivedRange ranges[DERIVED_MAX_RANGES];
   SelectSink sinks[SILO_GPU_MAX_SCAN_BATCH];  // k_finish_scan<true, n_scan> only
};
static_assert(sizeof(DerivedArgs) <= 4096, "the kernels of the derived symbols take their arguments by value: the kernel-argument segment holds 4 KiB");

/// The private tables of a scan with derived symbols and what its extra passes read, DERIVED_MAX_RANGES ranges at a time.
struct DerivedPlan {
   std::vector<DerivedArgs> launches;     // ranges [16 k, 16 k + 16) of the scan
   std::vector<ScanRange> private_ranges;  // the ranges with their count tables replaced by the private ones
   // every store with derived symbols has its gap events: the escape pass counts them into the gap tables (gap_ranges, one per
   // range, seqstore null where it has none) and none of the passes of the runs and the sparse keys runs
   bool events = false;
   std::vector<ScanRange> gap_ranges;
   // Which ranges count the end runs of the gap symbol instead of reading its covered rows (SeqStoreHost::Layout::ends):
   // decided ONCE per scan and range (usesEndRuns), whatever the proportions, the partitions or the entry — the counts are exact.
   // The row kernel and the gather kernel leave the covered rows out, the escape pass counts the end events into end_ranges (counts =
   // the range's ends tables; seqstore null where the range reads its rows) and the residual keys into the private tables,
   // k_finish_scan adds the end runs to the gap symbol's cell at the covered positions.
   std::vector<uint8_t> end_runs;
   std::vector<ScanRange> end_ranges;
   bool ends_apart = false;  // SILO_GPU_TUNE_END_RUNS = 1: the end events and residual keys in a launch of their own behind the row launch
   std::vector<std::array<uint64_t, DERIVED_MAX_RANGES>> run_counts;  // [launch][range] runs of the missing symbol of the range's store (for the timing log)
   size_t table_words = 0;       // zeroed by the prepare step: the tables, then the flags of the run parts
   size_t part_words = 0;        // behind them, not zeroed: the run parts (k_scan_missing_runs -> k_sum_run_parts)
   uint32_t most_positions = 0;  // of a range with derived symbols
   bool select = false;          // the finish launches overwrite the callers' tables and deliver the selected rows (SelectSink)
};

/// What a scan that selects (silo_gpu_mutations_scan_select, fused route) hands to scanRanges: per filter of the scan its sink
/// (total_blocks is filled in by planDerived), per range its first position in the filters' tables.
struct ScanSelect {
   SelectSink sinks[SILO_GPU_MAX_SCAN_BATCH];
   std::vector<uint32_t> table_offset;  // [range]
};

/// What a scan for Mutations rows of at least a proportion (silo_gpu_mutations_scan_ranges_min_proportion) may leave out: the keys
/// and rows that no reported row can come from (granulePrunable), their counts landing on the position's derived symbol.  Decided
/// ONCE per scan (scanRanges); the passes are handed this struct, or a null pointer for an exact scan.  Nothing is left out unless
/// some filter has a proportion in (0, 1] AND the scan counts gap events (DerivedPlan::events: only then does k_finish_scan
/// complete the tables); then SILO_GPU_TUNE_PRUNE_KEYS (g_tune_prune_keys) chooses: < 0 nothing, 0 keys and rows, 1 keys only.
struct ScanPruning {
   const uint32_t* counters;      // of the prepare step: [q * SPARSE_COUNTER_STRIDE + 2] = the cardinality of filter q
   const double* min_proportion;  // one per filter of the scan
   bool keys;                     // granules of escape keys (k_scan_escapes_sliced)
   bool rows;                     // one-hot plane rows (k_scan_sliced<.., KIND_ROWS>)
};

// the timing log of a scan (silo_gpu_scan.hip; SILO_GPU_TUNE_SCAN_TIMING, silo_gpu_scan_timings)
struct ScanLaunchTiming;
ScanLaunchTiming* startLaunchTiming(const char* kernel, uint64_t plane_rows, uint64_t bytes, uint32_t filters, uint32_t blocks, hipStream_t stream);
void finishLaunchTiming(ScanLaunchTiming* timing, hipStream_t stream);

// silo_gpu_scan_planes.hip
int scanShortRows(const std::vector<ScanRange>& ranges, bool nucleotide, const uint64_t* const* filters, uint32_t q_count, hipStream_t hip_stream);
hipError_t prepareScan(const uint64_t* const* filters, uint32_t q_count,
   uint32_t row_words, uint32_t capacity, uint32_t* counters, uint32_t* sector_index, uint32_t* tables, uint32_t table_words, uint32_t* counters_to_reset, hipStream_t hip_stream);
int scanPiecesDense(const std::vector<ScanPiece> (&pieces)[N_SCAN_LAYOUTS], const SeqStoreDev& any_store, const uint64_t* const* filters, uint32_t q_count,
   const uint32_t* sparse_sectors, uint32_t sparse_capacity, hipStream_t hip_stream, const ScanPruning* pruning);
int scanPiecesGather(const std::vector<ScanPiece> (&pieces)[N_SCAN_LAYOUTS], const SeqStoreDev& any_store, const uint64_t* const* filters, uint32_t q_count,
   const uint32_t* sparse_sectors, uint32_t sparse_capacity, const uint32_t* sector_index, uint32_t stride, hipStream_t hip_stream);

// silo_gpu_scan_keys.hip
extern thread_local uint32_t g_last_escape_items;  // items of the thread's last launch of k_scan_escapes_sliced (silo_gpu_last_escape_items)
int scanEscapes(const std::vector<ScanRange>& ranges, const uint64_t* const* filters, uint32_t q_count, hipStream_t hip_stream, const std::vector<ScanRange>* gaps, const ScanPruning* pruning,
   const std::vector<ScanRange>* ends = nullptr, bool only_ends = false);

// silo_gpu_scan_derived.hip
bool derivedCountsEvents(const std::vector<ScanRange>& ranges);
void planDerived(const silo_gpu_store* store, const std::vector<ScanRange>& ranges, const uint64_t* const* filters, uint32_t q_count, DerivedPlan& plan,
   const ScanSelect* select = nullptr);
void bindDerived(DerivedPlan& plan, uint32_t* tables, const uint32_t* counters, uint32_t q_count);
int scanRowsWithoutSymbol(DerivedPlan& plan, uint32_t q_count, hipStream_t hip_stream);
int finishDerived(DerivedPlan& plan, uint32_t q_count, hipStream_t hip_stream);

}  // namespace silo_gpu_detail
