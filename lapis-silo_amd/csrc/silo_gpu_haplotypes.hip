// silo_gpu_haplotypes.hip — K16, the symbol columns behind Haplotypes / AminoAcidHaplotypes.
//
// silo_gpu_position_symbols: the symbol id of EVERY row at up to SILO_GPU_MAX_HAPLOTYPE_POSITIONS listed positions, one byte per
// (position, row), read off the store's own layout — one pass per kind of stored thing, the decomposition of K7 and K11, here per
// cell instead of counted:
//   k_symbols_planes        the plane rows: a thread per row, a wave per row word; the valid symbol of the row's code, the derived
//                           symbol of a LAYOUT_IMPLICIT position, the extra planes; SILO_GPU_SYMBOL_NONE where nothing claims the row
//   k_symbols_escapes       a thread per escape key of the listed positions' ranges of the position-major list
//   k_symbols_missing_runs  a thread per run of the missing symbol: the listed positions inside [start, end)
//   k_symbols_sparse_keys   a thread per sparse key (ambiguity code) of the listed positions' ranges
//   k_symbols_unresolved    counts the bytes of real rows that are still SILO_GPU_SYMBOL_NONE
// silo_gpu_haplotype_ids: such columns as mixed-radix tuple ids, SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN positions per uint32
// column, for silo_gpu_group_count / silo_gpu_group_count_hashed; and the rows of a filter whose listed symbols are all complete:
//   k_haplotype_ids         a thread per row, a wave's ballot per word of the row bitset
#include <algorithm>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t SYMBOL_THREADS = 256;  // rows of a block: rows are whole 256-byte lines, so the grids are exact
constexpr uint32_t SYMBOL_WAVES = SYMBOL_THREADS / 64u;
constexpr uint32_t MAX_LISTED = SILO_GPU_MAX_HAPLOTYPE_POSITIONS;
constexpr uint32_t PER_COLUMN = SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN;
constexpr uint32_t MAX_ID_COLUMNS = (MAX_LISTED + PER_COLUMN - 1u) / PER_COLUMN;
constexpr uint32_t MAX_EXTRA = 16;
constexpr uint8_t NONE = SILO_GPU_SYMBOL_NONE;
static_assert(MAX_LISTED <= 16, "a set of columns is a 16-bit mask");

struct SymbolArgs {
   SeqStoreDev dev;
   uint8_t* out;              // [n_listed][rows]
   uint32_t* unresolved;
   uint32_t rows;             // row_words * 64
   uint32_t sequence_count;
   uint32_t n_listed;
   uint32_t listed[MAX_LISTED];  // the positions, in request order
   // the distinct positions in ascending order, and the columns of `out` each one fills (a position may be listed twice)
   uint32_t n_distinct;
   uint32_t distinct[MAX_LISTED];
   uint32_t columns_of[MAX_LISTED];
   // scan symbol index -> symbol id, a byte each, eight to a word: a lookup is two shifts, never an indexed private array
   uint64_t symbol_of_scan[4];
   uint32_t n_extra;
   uint8_t extra_symbols[MAX_EXTRA];  // symbols kept in extra planes (none of them a valid symbol)
};

/// The key ranges of the distinct positions, back to back: thread t of a key pass owns key begin[i] + (t - first[i]) of the
/// i-th distinct position, where first[i] <= t < first[i + 1].
struct KeyRanges {
   uint32_t begin[MAX_LISTED];
   uint32_t first[MAX_LISTED + 1];
};

__device__ __forceinline__ uint8_t symbolOfScan(const SymbolArgs& args, uint32_t scan_index) {
   const uint64_t word = scan_index < 8u ? args.symbol_of_scan[0] : scan_index < 16u ? args.symbol_of_scan[1] : scan_index < 24u ? args.symbol_of_scan[2] : args.symbol_of_scan[3];
   return static_cast<uint8_t>(word >> ((scan_index & 7u) * 8u));
}

/// Writes `symbol` into row `row` of every column in the set `columns`.  row < sequence_count <= rows and a column of the set is
/// below n_listed (the host builds the sets), so the byte is inside `out`.
__device__ __forceinline__ void storeSymbol(const SymbolArgs& args, uint32_t columns, uint32_t row, uint8_t symbol) {
   for (uint32_t c = 0; c < args.n_listed; ++c) {
      if (((columns >> c) & 1u) != 0) {
         args.out[static_cast<size_t>(c) * args.rows + row] = symbol;
      }
   }
}

/// grid = (rows / 256, n_listed): block (x, c) writes rows [256 x, 256 x + 256) of column c, one thread per row.  A wave is one
/// row word: every plane word it needs is one wave-uniform 8-byte load (the word index is made uniform, so the loads are scalar),
/// its store 64 consecutive bytes.  Every byte of the column is written here; the override passes then replace single bytes.
__global__ __launch_bounds__(SYMBOL_THREADS) void k_symbols_planes(const SymbolArgs args) {
   const uint32_t row = blockIdx.x * SYMBOL_THREADS + threadIdx.x;  // < rows: the grid is exact
   const uint32_t column = blockIdx.y;
   const uint32_t position = args.listed[column];
   const uint32_t word = __builtin_amdgcn_readfirstlane(row >> 6);
   const uint32_t bit = row & 63u;
   const uint32_t row_words = args.dev.row_words;
   uint8_t symbol = NONE;
   if (row < args.sequence_count) {
      const PositionLayout layout = layoutOf(args.dev, position);
      const uint32_t code = codeOfRow(layout, row_words, word, bit);
      if (code != 0) {
         symbol = symbolOfScan(args, layout.identity ? code - 1u : layout.map[code]);
      } else if (layout.implicit) {  // no one-hot row claims the row: the derived symbol, until a key, a run or a code says otherwise
         symbol = symbolOfScan(args, layout.map[IMPLICIT_SLOT]);
      }
      for (uint32_t e = 0; e < args.n_extra; ++e) {  // (uniform) a symbol without a code that has a plane of its own
         const uint32_t extra = args.extra_symbols[e];
         if (((planePtr(args.dev, position, extra)[word] >> bit) & 1ull) != 0) {
            symbol = static_cast<uint8_t>(extra);
         }
      }
   }
   args.out[static_cast<size_t>(column) * args.rows + row] = symbol;
}

/// The distinct position whose range thread t falls in: the ranges are back to back, first[] ascending.
__device__ __forceinline__ uint32_t rangeOf(const KeyRanges& ranges, uint32_t n_distinct, uint32_t t) {
   uint32_t i = 0;
   while (i + 1u < n_distinct && t >= ranges.first[i + 1u]) {
      ++i;
   }
   return i;
}

/// A thread per escape key of the listed positions: a row's valid symbol that has neither a code nor a row at its position.
/// Nothing read from a key is used as an index before it is checked: the key's position must be the one whose range it was read
/// from (a listed one), its row a real row, its scan symbol one the store has — k_query_escapes is the model.
__global__ __launch_bounds__(256) void k_symbols_escapes(const SymbolArgs args, const KeyRanges ranges) {
   const uint32_t t = blockIdx.x * 256u + threadIdx.x;
   if (t >= ranges.first[args.n_distinct]) {
      return;
   }
   const uint32_t i = rangeOf(ranges, args.n_distinct, t);
   const uint64_t key = args.dev.escapes[ranges.begin[i] + (t - ranges.first[i])];
   const uint32_t position = static_cast<uint32_t>(key >> 37);
   const uint32_t scan_index = static_cast<uint32_t>(key >> 32) & 31u;
   const uint32_t row = static_cast<uint32_t>(key);
   if (position != args.distinct[i] || row >= args.sequence_count || scan_index >= args.dev.n_scan) {
      return;
   }
   storeSymbol(args, args.columns_of[i], row, symbolOfScan(args, scan_index));
}

/// A thread per run of the missing symbol: the listed positions inside [start, end), found by a binary search of the <= 12
/// distinct positions in the kernel arguments.
__global__ __launch_bounds__(256) void k_symbols_missing_runs(const SymbolArgs args) {
   const uint32_t run = blockIdx.x * 256u + threadIdx.x;
   if (run >= args.dev.n_missing_runs) {
      return;
   }
   const uint64_t key = args.dev.missing_run_keys[run];
   const uint32_t row = static_cast<uint32_t>(key >> 32);
   const uint32_t start = static_cast<uint32_t>(key);
   const uint32_t end = min(args.dev.missing_run_ends[run], args.dev.positions);
   if (row >= args.sequence_count || start >= end) {
      return;
   }
   uint32_t lo = 0, hi = args.n_distinct;
   while (lo < hi) {  // the first distinct position at or past start
      const uint32_t mid = (lo + hi) / 2u;
      if (args.distinct[mid] < start) {
         lo = mid + 1u;
      } else {
         hi = mid;
      }
   }
   for (uint32_t i = lo; i < args.n_distinct && args.distinct[i] < end; ++i) {
      storeSymbol(args, args.columns_of[i], row, static_cast<uint8_t>(args.dev.missing_symbol));
   }
}

/// A thread per sparse key of the listed positions: an ambiguity code, or the missing symbol where it has neither runs nor a
/// plane.  The same checks as for an escape key; the symbol of a sparse key is a symbol id already.
__global__ __launch_bounds__(256) void k_symbols_sparse_keys(const SymbolArgs args, const uint64_t* __restrict__ sparse_keys, const KeyRanges ranges) {
   const uint32_t t = blockIdx.x * 256u + threadIdx.x;
   if (t >= ranges.first[args.n_distinct]) {
      return;
   }
   const uint32_t i = rangeOf(ranges, args.n_distinct, t);
   const uint64_t key = sparse_keys[ranges.begin[i] + (t - ranges.first[i])];
   const uint32_t position = static_cast<uint32_t>(key >> 37);
   const uint32_t symbol = static_cast<uint32_t>(key >> 32) & 31u;
   const uint32_t row = static_cast<uint32_t>(key);
   if (position != args.distinct[i] || row >= args.sequence_count || symbol >= args.dev.n_symbols) {
      return;
   }
   storeSymbol(args, args.columns_of[i], row, static_cast<uint8_t>(symbol));
}

/// grid = (rows / 256, n_listed), a thread per byte: the real rows still without a symbol.  A ballot per wave, the waves' counts
/// through LDS, one integer add per block that found any — into a word the entry has cleared on the same stream.
__global__ __launch_bounds__(SYMBOL_THREADS) void k_symbols_unresolved(const SymbolArgs args) {
   __shared__ uint32_t s_waves[SYMBOL_WAVES];
   const uint32_t row = blockIdx.x * SYMBOL_THREADS + threadIdx.x;
   const bool none = row < args.sequence_count && args.out[static_cast<size_t>(blockIdx.y) * args.rows + row] == NONE;
   const auto lanes = static_cast<uint32_t>(__popcll(__ballot(none)));
   if ((threadIdx.x & 63u) == 0) {
      s_waves[threadIdx.x / 64u] = lanes;
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t w = 0; w < SYMBOL_WAVES; ++w) {
         sum += s_waves[w];
      }
      if (sum != 0) {
         atomicAdd(args.unresolved, sum);
      }
   }
}

struct IdArgs {
   const uint8_t* symbols;  // [n_listed][rows]
   const uint64_t* filter;  // nullptr = all rows
   uint32_t* ids[MAX_ID_COLUMNS];
   uint64_t* out_rows;      // nullptr = not wanted
   uint32_t rows;
   uint32_t sequence_count;
   uint32_t n_listed;
   uint32_t n_symbols;
   uint32_t complete_symbols;
};

/// grid = rows / 256, a thread per row.  The row's bytes are read column by column (a wave reads 64 consecutive bytes of each).
/// A byte at or past n_symbols — SILO_GPU_SYMBOL_NONE, or anything else no symbol id can be — makes the row's ids 0 in every
/// column: an id is an index of the count kernels' tables and stays below n_symbols^m whatever the bytes hold.
__global__ __launch_bounds__(SYMBOL_THREADS) void k_haplotype_ids(const IdArgs args) {
   const uint32_t row = blockIdx.x * SYMBOL_THREADS + threadIdx.x;
   if (row >= args.rows) {
      return;  // (whole waves: rows is a multiple of 64)
   }
   const bool real = row < args.sequence_count;
   bool known = real;
   bool complete = real;
   uint32_t ids[MAX_ID_COLUMNS];
#pragma unroll
   for (uint32_t j = 0; j < MAX_ID_COLUMNS; ++j) {
      uint32_t id = 0;
      if (real) {
         const uint32_t column_begin = j * PER_COLUMN;
         const uint32_t column_end = min(args.n_listed, column_begin + PER_COLUMN);
         for (uint32_t c = column_begin; c < column_end; ++c) {
            const uint32_t symbol = args.symbols[static_cast<size_t>(c) * args.rows + row];
            known = known && symbol < args.n_symbols;
            // (a byte of 32 or more is no bit of the mask: complete only where the mask leaves nothing out)
            complete = complete && (symbol < 32u ? ((args.complete_symbols >> symbol) & 1u) != 0 : args.complete_symbols == 0xFFFFFFFFu);
            id = id * args.n_symbols + (symbol < args.n_symbols ? symbol : 0u);
         }
      }
      ids[j] = id;
   }
#pragma unroll
   for (uint32_t j = 0; j < MAX_ID_COLUMNS; ++j) {
      if (j * PER_COLUMN < args.n_listed) {
         args.ids[j][row] = known ? ids[j] : 0u;
      }
   }
   if (args.out_rows != nullptr) {  // (uniform)
      const uint32_t word = row >> 6;
      const bool selected = complete && (args.filter == nullptr || ((args.filter[word] >> (row & 63u)) & 1ull) != 0);
      const uint64_t bits = __ballot(selected);
      if ((threadIdx.x & 63u) == 0) {
         args.out_rows[word] = bits;
      }
   }
}

uint32_t blocksOf(uint32_t items) {
   return (items + 255u) / 256u;
}

}  // namespace

extern "C" {

int silo_gpu_position_symbols(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint32_t* positions, uint32_t n_positions, uint8_t* out_symbols_dev,
   uint32_t* out_unresolved_dev, void* stream
) {
   if (store == nullptr || positions == nullptr || out_symbols_dev == nullptr || out_unresolved_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_position_symbols: a pointer is NULL");
   }
   if (seqstore_id >= store->seqstores.size()) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_position_symbols: seqstore_id out of range");
   }
   if (n_positions == 0 || n_positions > MAX_LISTED) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_position_symbols: n_positions is 0 or above SILO_GPU_MAX_HAPLOTYPE_POSITIONS");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (!seqstore.finalized || dev.planes == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_position_symbols: store not finalized");
   }
   for (uint32_t c = 0; c < n_positions; ++c) {
      if (positions[c] >= dev.positions) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_position_symbols: position out of range");
      }
   }
   if (dev.n_symbols > 32u || dev.n_scan > 32u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_position_symbols: more symbols than a key holds");  // (cannot happen)
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);

   SymbolArgs args{};
   args.dev = dev;
   args.out = out_symbols_dev;
   args.unresolved = out_unresolved_dev;
   args.rows = dev.row_words * 64u;  // a multiple of SYMBOL_THREADS (rows are whole 256-byte lines)
   args.sequence_count = std::min(store->sequence_count, args.rows);
   args.n_listed = n_positions;
   std::copy(positions, positions + n_positions, args.listed);
   std::copy(positions, positions + n_positions, args.distinct);
   std::sort(args.distinct, args.distinct + n_positions);
   args.n_distinct = static_cast<uint32_t>(std::unique(args.distinct, args.distinct + n_positions) - args.distinct);
   for (uint32_t i = 0; i < args.n_distinct; ++i) {
      for (uint32_t c = 0; c < n_positions; ++c) {
         args.columns_of[i] |= positions[c] == args.distinct[i] ? 1u << c : 0u;
      }
   }
   for (uint32_t scan_index = 0; scan_index < 32u; ++scan_index) {
      args.symbol_of_scan[scan_index / 8u] |= static_cast<uint64_t>(NONE) << ((scan_index % 8u) * 8u);
   }
   for (uint32_t s = 0; s < dev.n_symbols; ++s) {
      if (dev.kind[s] == PLANE_SCAN && dev.index[s] < 32u) {
         uint64_t& word = args.symbol_of_scan[dev.index[s] / 8u];
         const uint32_t shift = (dev.index[s] % 8u) * 8u;
         word = (word & ~(0xFFull << shift)) | (static_cast<uint64_t>(s) << shift);
      } else if (dev.kind[s] == PLANE_EXTRA && dev.extra != nullptr && args.n_extra < MAX_EXTRA) {
         args.extra_symbols[args.n_extra++] = static_cast<uint8_t>(s);
      }
   }

   HIP_TRY(hipMemsetAsync(out_unresolved_dev, 0, sizeof(uint32_t), hip_stream));
   if (args.rows == 0) {
      return SILO_GPU_OK;
   }
   const dim3 cell_grid(args.rows / SYMBOL_THREADS, n_positions);
   k_symbols_planes<<<cell_grid, SYMBOL_THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());

   // The override passes, plain byte stores.  A cell holds ONE symbol, and finalize stores every cell of the build-time planes in
   // exactly one place — a code or one-hot row bit, or an escape key (valid symbols: the layout re-encoding), a run of the
   // missing symbol or an extra plane bit, or a sparse key (every other symbol) — so no two keys or runs name the same cell, and
   // no two threads write the same byte; a LAYOUT_IMPLICIT position is chosen only where every row has a symbol at every
   // position (everyRowHasASymbol), so what nothing stored names there is the derived symbol the plane pass has written.
   const bool has_map = dev.code_map != nullptr && !seqstore.layout.code_map.empty();
   if (has_map && dev.escapes != nullptr && seqstore.layout.escape_first.size() == static_cast<size_t>(dev.positions) + 1u) {
      KeyRanges ranges{};
      for (uint32_t i = 0; i < args.n_distinct; ++i) {
         const uint32_t begin = seqstore.layout.escape_first[args.distinct[i]];
         const uint32_t end = std::max(begin, seqstore.layout.escape_first[args.distinct[i] + 1u]);
         ranges.begin[i] = begin;
         ranges.first[i + 1u] = ranges.first[i] + (end - begin);
      }
      if (const uint32_t keys = ranges.first[args.n_distinct]; keys != 0) {
         k_symbols_escapes<<<blocksOf(keys), 256, 0, hip_stream>>>(args, ranges);
         HIP_TRY(hipGetLastError());
      }
   }
   if (dev.kind[dev.missing_symbol] == PLANE_RUNS && dev.n_missing_runs != 0) {
      k_symbols_missing_runs<<<blocksOf(dev.n_missing_runs), 256, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (seqstore.d_sparse.get() != nullptr && !seqstore.sparse_sorted.empty()) {
      const std::vector<uint64_t>& sorted = seqstore.sparse_sorted;  // the host copy of d_sparse, as silo_gpu_store_sparse_plane reads it
      KeyRanges ranges{};
      for (uint32_t i = 0; i < args.n_distinct; ++i) {
         const auto lo = std::lower_bound(sorted.begin(), sorted.end(), static_cast<uint64_t>(args.distinct[i]) << 37);
         const auto hi = std::lower_bound(lo, sorted.end(), (static_cast<uint64_t>(args.distinct[i]) + 1u) << 37);
         ranges.begin[i] = static_cast<uint32_t>(lo - sorted.begin());
         ranges.first[i + 1u] = ranges.first[i] + static_cast<uint32_t>(hi - lo);
      }
      if (const uint32_t keys = ranges.first[args.n_distinct]; keys != 0) {
         k_symbols_sparse_keys<<<blocksOf(keys), 256, 0, hip_stream>>>(args, seqstore.d_sparse.get(), ranges);
         HIP_TRY(hipGetLastError());
      }
   }
   k_symbols_unresolved<<<cell_grid, SYMBOL_THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_haplotype_ids(
   const uint8_t* symbols_dev, uint32_t n_positions, uint32_t row_words, uint32_t sequence_count, uint32_t n_symbols, uint32_t complete_symbols,
   const uint64_t* filter_dev, uint32_t* const* out_ids_dev, uint64_t* out_rows_dev, void* stream
) {
   if (symbols_dev == nullptr || out_ids_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_haplotype_ids: a pointer is NULL");
   }
   if (n_positions == 0 || n_positions > MAX_LISTED) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_haplotype_ids: n_positions is 0 or above SILO_GPU_MAX_HAPLOTYPE_POSITIONS");
   }
   if (n_symbols == 0 || n_symbols > 32u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_haplotype_ids: n_symbols is 0 or above 32");
   }
   if (row_words == 0 || row_words > UINT32_MAX / 64u || sequence_count > row_words * 64u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_haplotype_ids: row_words is 0, or sequence_count above row_words * 64");
   }
   IdArgs args{};
   const uint32_t n_columns = (n_positions + PER_COLUMN - 1u) / PER_COLUMN;
   for (uint32_t j = 0; j < n_columns; ++j) {
      if (out_ids_dev[j] == nullptr) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_haplotype_ids: an id column is NULL");
      }
      args.ids[j] = out_ids_dev[j];
   }
   args.symbols = symbols_dev;
   args.filter = filter_dev;
   args.out_rows = out_rows_dev;
   args.rows = row_words * 64u;
   args.sequence_count = sequence_count;
   args.n_listed = n_positions;
   args.n_symbols = n_symbols;
   args.complete_symbols = complete_symbols;
   k_haplotype_ids<<<blocksOf(args.rows), SYMBOL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(args);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
