// silo_gpu_region_counts.hip — K23, the filter expression CellCount over a position range and the action CellCountByRegion
// (DESIGN.md §30): per row of a sequence store and per region [first, end) of positions, the number of the row's cells there whose
// class (cell_class.h, K22's) is one of the kinds of a mask.  It is K22's decomposition (row_fold.h) with a 0/1 weight in place of a
// class vector and with every pass confined to the regions:
//   k_region_value_planes    a wave per (row word, region), a lane per row, the region's positions only; what a cell holds is
//                            row_fold.h's cellSymbol; the value stays in a register and leaves with one 256-byte store per wave
//   k_region_value_escapes   a thread per escape key of the ranges' slices [escape_first[first], escape_first[end]) of the
//                            position-major keys; the slices of all ranges are flattened on the host into ONE index space (a
//                            launch per range would be up to 256 launches of a few keys each)
//   k_region_value_sparse    the same over the ranges' slices of the sorted sparse keys, found by a host binary search
//   k_region_value_runs      a thread per run of the missing symbol: for each region the run meets, two lookups in a prefix
//                            array clipped to the region and at most one atomic
// Each correction adds in(class now) - in(class the plane pass assumed), mod 2^32: exact whatever the schedule.
// The two readers of such columns take no store:
//   k_bitset_from_values     a thread per row, a wave's ballot per word
//   k_count_values           per column: a wave per filter word (grid-stride), ballot and popcount, a block sum, one 64-bit add
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "cell_class.h"
#include "row_fold.h"
#include "store_internal.h"

using namespace silo_gpu_detail;
using namespace silo_gpu_row_fold;
using namespace silo_gpu_cell_class;

namespace {

constexpr uint32_t THREADS = 256;  // four waves
constexpr uint32_t WORDS_PER_BLOCK = THREADS / 64u;
constexpr uint32_t MAX_REGIONS = SILO_GPU_MAX_REGIONS;
constexpr uint32_t MAX_COUNT_BLOCKS = 1024;  // per column
constexpr uint16_t NO_REGION = 0xFFFFu;
static_assert(MAX_REGIONS < NO_REGION);

/// A region as the passes read it: its positions, and where its slices of the two key lists sit in the lists and in the
/// flattened index spaces of the escape and the sparse pass.
struct RegionSlices {
   uint32_t first, end;               // positions [first, end)
   uint32_t escape_begin, escape_at;  // its escape keys start at escapes[escape_begin]; they are items [escape_at, next region's escape_at)
   uint32_t sparse_begin, sparse_at;  // the same for the sparse keys
};

/// What the four passes share beside LayoutArgs.
struct RegionArgs {
   const uint8_t* reference;      // [P] symbol indices
   const uint16_t* region_of;     // [P] the region of a position, or NO_REGION
   const RegionSlices* regions;   // [n_regions]
   const uint32_t* run_prefix;    // [P + 1] sums over q < p inside a region of in(MISSING) - in(class(q, base_symbol[q]))
   uint32_t* values;              // [n_regions][row_words * 64]
   uint32_t n_regions;
   uint32_t n_escape_items;       // keys of all slices
   uint32_t n_sparse_items;
   uint32_t kinds_mask;
   uint32_t valid;                // the alphabet's valid mutation symbols
   uint32_t missing;
};

/// 1 where the class of `symbol` at a position whose reference symbol is `reference` is one of the kinds of the mask.
__host__ __device__ __forceinline__ uint32_t weightOf(uint32_t symbol, uint32_t reference, uint32_t missing, uint32_t valid, uint32_t kinds_mask) {
   const uint32_t cell_class = classOf(symbol, reference, missing, valid);
   return cell_class != SAME ? (kinds_mask >> cell_class) & 1u : 0u;
}

/// Turns the cell of (row, position) from `base` into `symbol` in the column of the position's region.
__device__ __forceinline__ void correctCell(const LayoutArgs& args, const RegionArgs& region_args, uint32_t row, uint32_t position, uint32_t symbol) {
   const uint32_t region = region_args.region_of[position];
   if (region >= region_args.n_regions) {
      return;  // (a key of a slice lies inside its region: cannot happen)
   }
   const uint32_t reference = region_args.reference[position];
   const uint32_t now = weightOf(symbol, reference, region_args.missing, region_args.valid, region_args.kinds_mask);
   const uint32_t before = weightOf(args.base_symbol[position], reference, region_args.missing, region_args.valid, region_args.kinds_mask);
   if (now != before) {
      atomicAdd(region_args.values + static_cast<size_t>(region) * args.dev.row_words * 64u + row, now - before);
   }
}

/// The region whose items hold item `item` of a flattened index space: the last region whose first item (`escape_at` or `sparse_at`)
/// is <= item.  Regions without items share their first item with the next one and are passed over.
template <uint32_t RegionSlices::*AT>
__device__ __forceinline__ uint32_t regionOfItem(const RegionArgs& region_args, uint32_t item) {
   uint32_t low = 0;
   uint32_t high = region_args.n_regions;  // the answer is in [low, high)
   while (high - low > 1u) {
      const uint32_t middle = (low + high) / 2u;
      if (region_args.regions[middle].*AT <= item) {
         low = middle;
      } else {
         high = middle;
      }
   }
   return low;
}

/// grid = n_regions * row_words waves, FOLD_WORDS_PER_BLOCK to a block, the row words of a region next to each other.
__global__ __launch_bounds__(FOLD_THREADS) void k_region_value_planes(const LayoutArgs args, const RegionArgs region_args) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   const uint32_t row_words = args.dev.row_words;
   const uint64_t pair = static_cast<uint64_t>(blockIdx.x) * FOLD_WORDS_PER_BLOCK + (threadIdx.x >> 6);
   const uint32_t region = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(pair / row_words));  // (uniform over the wave)
   const uint32_t word = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(pair % row_words));
   if (region >= region_args.n_regions) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const bool has_extra = args.n_extra != 0 && args.dev.extra != nullptr;
   const uint32_t end = min(region_args.regions[region].end, args.dev.positions);
   uint32_t value = 0;
   for (uint32_t position = region_args.regions[region].first; position < end; ++position) {
      const uint32_t symbol = cellSymbol(args, s_symbol_of_scan, position, word, lane, has_extra);
      value += weightOf(symbol, region_args.reference[position], region_args.missing, region_args.valid, region_args.kinds_mask);
   }
   const uint64_t row = static_cast<uint64_t>(word) * 64u + lane;
   region_args.values[static_cast<size_t>(region) * row_words * 64u + row] = row < args.sequence_count ? value : 0u;
}

/// A thread per escape key of the ranges' slices (grid-stride over the flattened items).
__global__ __launch_bounds__(FOLD_THREADS) void k_region_value_escapes(const LayoutArgs args, const RegionArgs region_args) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   for (uint32_t item = blockIdx.x * FOLD_THREADS + threadIdx.x; item < region_args.n_escape_items; item += gridDim.x * FOLD_THREADS) {
      const RegionSlices slices = region_args.regions[regionOfItem<&RegionSlices::escape_at>(region_args, item)];
      const uint32_t i = slices.escape_begin + (item - slices.escape_at);
      if (i >= args.n_escapes) {
         continue;  // (cannot happen)
      }
      const uint64_t key = args.dev.escapes[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t symbol = s_symbol_of_scan[static_cast<uint32_t>(key >> 32) & 31u];
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count && symbol != NO_SCAN_SYMBOL) {
         correctCell(args, region_args, row, position, symbol);
      }
   }
}

/// A thread per sparse key of the ranges' slices (grid-stride over the flattened items).
__global__ __launch_bounds__(FOLD_THREADS) void k_region_value_sparse(const LayoutArgs args, const RegionArgs region_args) {
   for (uint32_t item = blockIdx.x * FOLD_THREADS + threadIdx.x; item < region_args.n_sparse_items; item += gridDim.x * FOLD_THREADS) {
      const RegionSlices slices = region_args.regions[regionOfItem<&RegionSlices::sparse_at>(region_args, item)];
      const uint32_t i = slices.sparse_begin + (item - slices.sparse_at);
      if (i >= args.n_sparse) {
         continue;  // (cannot happen)
      }
      const uint64_t key = args.sparse_keys[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count) {
         correctCell(args, region_args, row, position, static_cast<uint32_t>(key >> 32) & 31u);
      }
   }
}

/// A thread per run [start, end) of the missing symbol (grid-stride).  The first region the run can meet is the one `start` lies
/// in (region_of), or else the first that begins behind it (a binary search of the ascending ranges); from there onwards while
/// the region begins before `end`.
__global__ __launch_bounds__(FOLD_THREADS) void k_region_value_runs(const LayoutArgs args, const RegionArgs region_args) {
   for (uint32_t i = blockIdx.x * FOLD_THREADS + threadIdx.x; i < args.dev.n_missing_runs; i += gridDim.x * FOLD_THREADS) {
      const uint64_t key = args.dev.missing_run_keys[i];
      const uint32_t row = static_cast<uint32_t>(key >> 32);
      const uint32_t start = static_cast<uint32_t>(key);
      const uint32_t end = min(args.dev.missing_run_ends[i], args.dev.positions);
      if (start >= end || row >= args.sequence_count) {
         continue;
      }
      uint32_t region = region_args.region_of[start];
      if (region >= region_args.n_regions) {
         uint32_t low = 0;
         uint32_t high = region_args.n_regions;  // the first region with first > start is in [low, high]
         while (low < high) {
            const uint32_t middle = (low + high) / 2u;
            if (region_args.regions[middle].first > start) {
               high = middle;
            } else {
               low = middle + 1u;
            }
         }
         region = low;
      }
      for (; region < region_args.n_regions && region_args.regions[region].first < end; ++region) {
         const uint32_t from = max(start, region_args.regions[region].first);
         const uint32_t to = min(end, region_args.regions[region].end);
         const uint32_t difference = from < to ? region_args.run_prefix[to] - region_args.run_prefix[from] : 0u;
         if (difference != 0) {
            atomicAdd(region_args.values + static_cast<size_t>(region) * args.dev.row_words * 64u + row, difference);
         }
      }
   }
}

// ---- the readers of columns ------------------------------------------------------------------------------
/// A thread per row of one column, a wave per word of the bitset: one 4-byte load per lane, the wave's ballot of the predicate is
/// the word, stored by its first lane.  A wave whose word is at or past row_words neither loads nor stores; rows at or past
/// sequence_count give 0 whatever their cell holds.
__global__ __launch_bounds__(THREADS) void k_bitset_from_values(
   const uint32_t* __restrict__ values, uint32_t row_words, uint32_t sequence_count, uint32_t at_least, uint32_t at_most, uint64_t* __restrict__ out
) {
   const size_t row = static_cast<size_t>(blockIdx.x) * THREADS + threadIdx.x;
   const size_t word = row >> 6;  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint32_t value = values[row];
   const bool selected = row < sequence_count && value >= at_least && value <= at_most;
   const uint64_t bits = __ballot(selected);
   if ((threadIdx.x & 63u) == 0) {
      out[word] = bits;
   }
}

/// The bounds of every column, passed by value (2 KiB of kernel arguments): no upload, nothing to keep alive.
struct ColumnBounds {
   uint32_t bound[MAX_REGIONS][2];
};

/// grid = (blocks <= MAX_COUNT_BLOCKS, n_columns); in column blockIdx.y a wave takes the filter words wave, wave + waves of the
/// grid's row, ...
__global__ __launch_bounds__(THREADS) void k_count_values(
   const uint32_t* __restrict__ values, uint32_t row_words, uint32_t sequence_count, const uint64_t* __restrict__ filter, const ColumnBounds bounds,
   unsigned long long* __restrict__ counts
) {
   __shared__ uint32_t s_wave_counts[WORDS_PER_BLOCK];
   const uint32_t column = blockIdx.y;
   const uint32_t at_least = bounds.bound[column][0];
   const uint32_t at_most = bounds.bound[column][1];
   const uint32_t* __restrict__ column_values = values + static_cast<size_t>(column) * row_words * 64u;
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK;
   uint32_t counted = 0;  // (uniform over the wave; a wave sees fewer than 2^32 rows)
   for (uint64_t word = static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6); word < row_words; word += step) {
      const uint64_t bits = filter != nullptr ? filter[word] : ~0ull;
      const uint64_t row = word * 64u + lane;
      bool inside = false;
      if (((bits >> lane) & 1ull) != 0 && row < sequence_count) {
         const uint32_t value = column_values[row];
         inside = value >= at_least && value <= at_most;
      }
      counted += static_cast<uint32_t>(__popcll(__ballot(inside)));
   }
   if (lane == 0) {
      s_wave_counts[threadIdx.x >> 6] = counted;
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t sum = 0;
      for (uint32_t wave = 0; wave < WORDS_PER_BLOCK; ++wave) {
         sum += s_wave_counts[wave];
      }
      if (sum != 0) {
         atomicAdd(counts + column, static_cast<unsigned long long>(sum));
      }
   }
}

int checkColumns(const char* entry, const void* values_dev, const void* out_dev, uint32_t row_words, uint32_t sequence_count) {
   if (values_dev == nullptr || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad arguments");
   }
   if (row_words == 0 || sequence_count == 0 || sequence_count > static_cast<uint64_t>(row_words) * 64u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": the columns have no rows, or fewer than sequence_count");
   }
   return SILO_GPU_OK;
}

}  // namespace

extern "C" {

int silo_gpu_region_cell_values(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint32_t* ranges, uint32_t n_ranges, uint32_t kinds_mask, uint32_t* values_dev,
   void* scratch_dev, void* stream
) {
   const char* const entry = "silo_gpu_region_cell_values";
   if (store == nullptr || seqstore_id >= store->seqstores.size() || ranges == nullptr || values_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad arguments");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (!seqstore.finalized || dev.planes == nullptr || dev.row_words == 0 || seqstore.d_reference.get() == nullptr ||
       seqstore.reference.size() != dev.positions) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": store is not finalized");
   }
   if (n_ranges == 0 || n_ranges > MAX_REGIONS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": n_ranges is 0 or above SILO_GPU_MAX_REGIONS");
   }
   if (kinds_mask == 0 || kinds_mask >= (1u << SILO_GPU_CELL_COUNT_KINDS)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": kinds_mask names no kind, or one that does not exist");
   }
   const uint32_t P = dev.positions;
   for (uint32_t g = 0; g < n_ranges; ++g) {
      const uint32_t first = ranges[2u * g];
      const uint32_t end = ranges[2u * g + 1u];
      if (first >= end || end > P || (g != 0 && first < ranges[2u * g - 1u])) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": a range is empty, out of order, overlapping or past the end of the sequence");
      }
   }
   const hipStream_t hip_stream = static_cast<hipStream_t>(stream);
   HIP_TRY(hipSetDevice(store->device));

   // the tables of the call: base_symbol[P] | region_of[P] | regions[n_ranges] | run_prefix[P + 1]
   const size_t base_bytes = align256(P);
   const size_t region_of_bytes = align256(static_cast<size_t>(P) * sizeof(uint16_t));
   const size_t regions_bytes = align256(static_cast<size_t>(n_ranges) * sizeof(RegionSlices));
   const size_t prefix_bytes = align256((static_cast<size_t>(P) + 1u) * sizeof(uint32_t));
   const size_t table_bytes = base_bytes + region_of_bytes + regions_bytes + prefix_bytes;
   if (table_bytes > SILO_GPU_REGION_VALUE_SCRATCH_BYTES(P)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": scratch layout exceeds its documented size");  // (cannot happen)
   }
   std::vector<uint8_t> tables(table_bytes, 0);
   uint8_t* t_base = tables.data();
   auto* t_region_of = reinterpret_cast<uint16_t*>(tables.data() + base_bytes);
   auto* t_regions = reinterpret_cast<RegionSlices*>(tables.data() + base_bytes + region_of_bytes);
   auto* t_prefix = reinterpret_cast<uint32_t*>(tables.data() + base_bytes + region_of_bytes + regions_bytes);
   fillBaseSymbols(seqstore, t_base);
   std::fill(t_region_of, t_region_of + P, NO_REGION);

   const uint32_t valid = seqstore.alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE ? VALID_NUCLEOTIDES : VALID_AMINO_ACIDS;
   LayoutArgs args = layoutArgsOf(store, seqstore, static_cast<const uint8_t*>(scratch_dev));
   const std::vector<uint64_t>& sparse = seqstore.sparse_sorted;
   const std::vector<uint32_t>& escape_first = seqstore.layout.escape_first;
   const bool has_escapes = args.n_escapes != 0 && escape_first.size() == static_cast<size_t>(P) + 1u;
   uint32_t escape_items = 0;
   uint32_t sparse_items = 0;
   for (uint32_t g = 0; g < n_ranges; ++g) {
      RegionSlices& region = t_regions[g];
      region.first = ranges[2u * g];
      region.end = ranges[2u * g + 1u];
      std::fill(t_region_of + region.first, t_region_of + region.end, static_cast<uint16_t>(g));
      region.escape_begin = has_escapes ? std::min(escape_first[region.first], args.n_escapes) : 0u;
      region.escape_at = escape_items;
      escape_items += has_escapes ? std::min(escape_first[region.end], args.n_escapes) - region.escape_begin : 0u;
      // sparse keys are position << 37 | symbol << 32 | sequence, ascending: the keys of [first, end) are one slice
      const auto slice_begin = std::lower_bound(sparse.begin(), sparse.begin() + args.n_sparse, static_cast<uint64_t>(region.first) << 37);
      const auto slice_end = std::lower_bound(slice_begin, sparse.begin() + args.n_sparse, static_cast<uint64_t>(region.end) << 37);
      region.sparse_begin = static_cast<uint32_t>(slice_begin - sparse.begin());
      region.sparse_at = sparse_items;
      sparse_items += static_cast<uint32_t>(slice_end - slice_begin);
   }
   const uint32_t missing = dev.missing_symbol;
   for (uint32_t p = 0; p < P; ++p) {
      uint32_t step = 0;
      if (t_region_of[p] != NO_REGION) {
         step = weightOf(missing, seqstore.reference[p], missing, valid, kinds_mask) - weightOf(t_base[p], seqstore.reference[p], missing, valid, kinds_mask);
      }
      t_prefix[p + 1u] = t_prefix[p] + step;
   }
   auto* scratch = static_cast<uint8_t*>(scratch_dev);
   HIP_TRY(hipMemcpyAsync(scratch, tables.data(), tables.size(), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   RegionArgs region_args{};
   region_args.reference = seqstore.d_reference.get();
   region_args.region_of = reinterpret_cast<const uint16_t*>(scratch + base_bytes);
   region_args.regions = reinterpret_cast<const RegionSlices*>(scratch + base_bytes + region_of_bytes);
   region_args.run_prefix = reinterpret_cast<const uint32_t*>(scratch + base_bytes + region_of_bytes + regions_bytes);
   region_args.values = values_dev;
   region_args.n_regions = n_ranges;
   region_args.n_escape_items = escape_items;
   region_args.n_sparse_items = sparse_items;
   region_args.kinds_mask = kinds_mask;
   region_args.valid = valid;
   region_args.missing = missing;

   const uint64_t pairs = static_cast<uint64_t>(n_ranges) * dev.row_words;  // <= 256 * 2^26 / 64: the grid fits
   const uint32_t plane_blocks = static_cast<uint32_t>((pairs + FOLD_WORDS_PER_BLOCK - 1u) / FOLD_WORDS_PER_BLOCK);
   k_region_value_planes<<<plane_blocks, FOLD_THREADS, 0, hip_stream>>>(args, region_args);
   HIP_TRY(hipGetLastError());
   if (escape_items != 0) {
      k_region_value_escapes<<<strideBlocks(escape_items, FOLD_THREADS), FOLD_THREADS, 0, hip_stream>>>(args, region_args);
      HIP_TRY(hipGetLastError());
   }
   if (dev.kind[dev.missing_symbol] == PLANE_RUNS && dev.n_missing_runs != 0 && dev.missing_run_keys != nullptr && dev.missing_run_ends != nullptr) {
      k_region_value_runs<<<strideBlocks(dev.n_missing_runs, FOLD_THREADS), FOLD_THREADS, 0, hip_stream>>>(args, region_args);
      HIP_TRY(hipGetLastError());
   }
   if (sparse_items != 0) {
      k_region_value_sparse<<<strideBlocks(sparse_items, FOLD_THREADS), FOLD_THREADS, 0, hip_stream>>>(args, region_args);
      HIP_TRY(hipGetLastError());
   }
   return SILO_GPU_OK;
}

int silo_gpu_bitset_from_values(
   const uint32_t* values_dev, uint32_t row_words, uint32_t sequence_count, uint32_t at_least, uint32_t at_most, uint64_t* out_bitset_dev, void* stream
) {
   if (const int status = checkColumns("silo_gpu_bitset_from_values", values_dev, out_bitset_dev, row_words, sequence_count); status != SILO_GPU_OK) {
      return status;
   }
   k_bitset_from_values<<<blocksOfWords(row_words, WORDS_PER_BLOCK), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      values_dev, row_words, sequence_count, at_least, at_most, out_bitset_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_count_values(
   const uint32_t* values_dev, uint32_t n_columns, uint32_t row_words, uint32_t sequence_count, const uint64_t* filter_dev, const uint32_t* bounds,
   uint64_t* counts_dev, void* stream
) {
   if (bounds == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_count_values: bad arguments");
   }
   if (const int status = checkColumns("silo_gpu_count_values", values_dev, counts_dev, row_words, sequence_count); status != SILO_GPU_OK) {
      return status;
   }
   if (n_columns == 0 || n_columns > MAX_REGIONS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_count_values: n_columns is 0 or above SILO_GPU_MAX_REGIONS");
   }
   ColumnBounds column_bounds{};
   std::copy(bounds, bounds + 2u * static_cast<size_t>(n_columns), &column_bounds.bound[0][0]);
   const dim3 grid(std::min(blocksOfWords(row_words, WORDS_PER_BLOCK), MAX_COUNT_BLOCKS), n_columns);
   k_count_values<<<grid, THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      values_dev, row_words, sequence_count, filter_dev, column_bounds, reinterpret_cast<unsigned long long*>(counts_dev)
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
