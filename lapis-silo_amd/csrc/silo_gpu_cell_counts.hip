// silo_gpu_cell_counts.hip — K22, the filter expression CellCount and the action CellCountDistribution: per row of a
// sequence store the number of its cells that are a substitution, a deletion, the missing symbol or ambiguous against the store's
// own reference — K18's four cell counts (silo_gpu_differences.hip), over all positions — kept by the store; a row bitset from a
// bound on the sum of some of the four; and the histogram of that sum over the selected rows.
// The counts are read off the store's layout as K20 reads its hashes (silo_gpu_distinct.hip), with class vectors — one of the four
// counts is 1, or none for a cell that equals the reference — in place of hash terms, mod 2^32:
//   k_cell_count_planes     a wave per row word, a lane per row, all positions: the lane's code at the position (code planes, one-hot
//                           rows, extra planes) selects the symbol, an open cell counts as the position's derived symbol or as 31;
//                           the four sums stay in registers and leave with one 16-byte store per row (zeros for padding rows)
//   k_cell_count_escapes    a thread per escape key: class(its symbol) - class(what the planes said), at most one -1 and one +1
//   k_cell_count_runs       a thread per run [a, e) of the missing symbol: two lookups in a prefix array of those differences
//   k_cell_count_sparse     a thread per sparse key (ambiguity code)
// The two readers of such a table take no store:
//   k_bitset_from_cell_counts  a thread per row, a wave's ballot per word
//   k_cell_count_histogram     a wave per filter word, a lane per selected row; a block's bins in LDS, flushed with 64-bit adds
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t THREADS = 256;  // four waves: four neighbouring row words per block
constexpr uint32_t WORDS_PER_BLOCK = THREADS / 64u;
constexpr uint32_t MAX_EXTRA = 16;
constexpr uint32_t SCAN_SLOTS = 32;  // scan symbol indices a key can name (5 bits)
constexpr uint8_t NO_SCAN_SYMBOL = 0xFF;
constexpr uint32_t NO_SYMBOL = SILO_GPU_ROW_HASH_NO_SYMBOL;  // a cell that nothing stored claims: ambiguous
constexpr uint32_t KINDS = SILO_GPU_CELL_COUNT_KINDS;
constexpr uint32_t MAX_BINS = SILO_GPU_MAX_CELL_COUNT_BINS;
constexpr uint32_t MAX_HISTOGRAM_BLOCKS = 2048;
static_assert(KINDS == SILO_GPU_DIFFERENCE_STATS && NO_SYMBOL >= SILO_GPU_MAX_SYMBOLS && NO_SYMBOL < 32u);

/// The class of a cell in K18's `stats` order; SAME counts nowhere.
enum CellClass : uint32_t { SUBSTITUTION = 0, DELETION = 1, MISSING = 2, AMBIGUOUS = 3, SAME = 4 };
constexpr uint32_t GAP_SYMBOL = 0;  // '-' in both alphabets

/// Bit s for every symbol index s that is a valid mutation symbol: -ACGT of "-ACGTRYSWKMBDHVN", and all of
/// "-ACDEFGHIKLMNPQRSTVWYBZ*X" but B, Z and X (fillCharTable, store_internal.h).
constexpr uint32_t VALID_NUCLEOTIDES = 0x1Fu;
constexpr uint32_t VALID_AMINO_ACIDS = 0x1FFFFFu | (1u << 23);

/// The class of the symbol index `symbol` (31: none) where the reference holds `reference`: K18's rule on indices.  A reference
/// symbol that is not valid equals no valid symbol.
__host__ __device__ __forceinline__ uint32_t classOf(uint32_t symbol, uint32_t reference, uint32_t missing, uint32_t valid) {
   if (symbol == missing) {
      return MISSING;
   }
   if (symbol >= 32u || ((valid >> symbol) & 1u) == 0) {
      return AMBIGUOUS;
   }
   if (symbol == reference) {
      return SAME;
   }
   return symbol == GAP_SYMBOL ? DELETION : SUBSTITUTION;
}

struct CellArgs {
   SeqStoreDev dev;
   const uint8_t* reference;     // [P] symbol indices
   const uint8_t* base_symbol;   // [P] what the plane pass takes an open cell for: the derived symbol, or NO_SYMBOL
   const uint32_t* run_prefix;   // [P + 1][4] sums over q < p of class(q, missing symbol) - class(q, base_symbol[q])
   const uint64_t* sparse_keys;
   uint32_t n_sparse;
   uint32_t n_escapes;
   uint32_t sequence_count;
   uint32_t valid;               // the alphabet's valid mutation symbols, a bit per symbol index
   uint32_t n_extra;
   uint8_t extra_symbols[MAX_EXTRA];  // symbols kept in extra planes
   uint32_t* out;                // [row_words * 64][4]
};

/// The symbol of every scan symbol index, in LDS (a lane looks its own code up): filled by the first SCAN_SLOTS threads.
__device__ __forceinline__ void fillSymbolOfScan(uint8_t* s_symbol_of_scan, const SeqStoreDev& dev) {
   if (threadIdx.x < SCAN_SLOTS) {
      uint32_t found = NO_SCAN_SYMBOL;
      for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {  // (uniform index: scalar loads)
         if (dev.kind[symbol] == PLANE_SCAN && dev.index[symbol] == threadIdx.x) {
            found = symbol;
         }
      }
      s_symbol_of_scan[threadIdx.x] = static_cast<uint8_t>(found);
   }
   __syncthreads();
}

/// grid = row_words / WORDS_PER_BLOCK rounded up.  The plane words of a position are the same for the whole wave: where all of
/// them are 0 — nearly always at a position that derives its symbol — every lane holds the position's base symbol and the
/// per-lane decode is skipped.
__global__ __launch_bounds__(THREADS) void k_cell_count_planes(const CellArgs args) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   const uint32_t row_words = args.dev.row_words;
   const uint32_t word = __builtin_amdgcn_readfirstlane(blockIdx.x * WORDS_PER_BLOCK + (threadIdx.x >> 6));  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t n_scan = args.dev.n_scan;
   const uint32_t missing = args.dev.missing_symbol;
   const bool has_extra = args.n_extra != 0 && args.dev.extra != nullptr;
   uint32_t counts[KINDS] = {0, 0, 0, 0};
   for (uint32_t position = 0; position < args.dev.positions; ++position) {
      const PositionLayout layout = layoutOf(args.dev, position);
      uint32_t code = 0;
      uint64_t any = 0;
      for (uint32_t plane = 0; plane < layout.bits; ++plane) {
         const uint64_t plane_word = layout.rows[static_cast<size_t>(plane) * row_words + word];
         any |= plane_word;
         const uint32_t set = static_cast<uint32_t>((plane_word >> lane) & 1ull);
         code = layout.one_hot ? (set != 0 ? plane + 1u : code) : (code | (set << plane));
      }
      uint32_t symbol = args.base_symbol[position];
      if (any != 0 && code != 0) {
         const uint32_t scan_index = layout.identity ? code - 1u : (code < CODE_MAP_STRIDE ? layout.map[code] : NO_SCAN_SYMBOL);
         if (scan_index < n_scan && scan_index < SCAN_SLOTS) {
            const uint32_t coded = s_symbol_of_scan[scan_index];
            symbol = coded != NO_SCAN_SYMBOL ? coded : symbol;
         }
      }
      if (has_extra) {
         for (uint32_t e = 0; e < args.n_extra; ++e) {
            const uint32_t extra_symbol = args.extra_symbols[e];
            if (((planePtr(args.dev, position, extra_symbol)[word] >> lane) & 1ull) != 0) {
               symbol = extra_symbol;
            }
         }
      }
      const uint32_t cell_class = classOf(symbol, args.reference[position], missing, args.valid);
#pragma unroll
      for (uint32_t k = 0; k < KINDS; ++k) {
         counts[k] += cell_class == k ? 1u : 0u;
      }
   }
   const uint64_t row = static_cast<uint64_t>(word) * 64u + lane;
   const bool real = row < args.sequence_count;
   reinterpret_cast<uint4*>(args.out)[row] = real ? make_uint4(counts[0], counts[1], counts[2], counts[3]) : make_uint4(0u, 0u, 0u, 0u);
}

/// Adds class(position, symbol) - class(position, base) to the row's cell: at most one +1 and one -1.
__device__ __forceinline__ void correct(const CellArgs& args, uint32_t row, uint32_t position, uint32_t symbol) {
   const uint32_t reference = args.reference[position];
   const uint32_t now = classOf(symbol, reference, args.dev.missing_symbol, args.valid);
   const uint32_t before = classOf(args.base_symbol[position], reference, args.dev.missing_symbol, args.valid);
   if (now == before) {
      return;
   }
   uint32_t* cell = args.out + static_cast<size_t>(KINDS) * row;
   if (now != SAME) {
      atomicAdd(cell + now, 1u);
   }
   if (before != SAME) {
      atomicAdd(cell + before, 0xFFFFFFFFu);
   }
}

/// A thread per escape key (grid-stride): a row's valid symbol that has neither a code nor a row at its position.
__global__ __launch_bounds__(THREADS) void k_cell_count_escapes(const CellArgs args) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < args.n_escapes; i += gridDim.x * THREADS) {
      const uint64_t key = args.dev.escapes[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t symbol = s_symbol_of_scan[static_cast<uint32_t>(key >> 32) & 31u];
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count && symbol != NO_SCAN_SYMBOL) {
         correct(args, row, position, symbol);
      }
   }
}

/// A thread per run of the missing symbol (grid-stride).
__global__ __launch_bounds__(THREADS) void k_cell_count_runs(const CellArgs args) {
   for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < args.dev.n_missing_runs; i += gridDim.x * THREADS) {
      const uint64_t key = args.dev.missing_run_keys[i];
      const uint32_t row = static_cast<uint32_t>(key >> 32);
      const uint32_t start = static_cast<uint32_t>(key);
      const uint32_t end = min(args.dev.missing_run_ends[i], args.dev.positions);
      if (start < end && row < args.sequence_count) {
         uint32_t* cell = args.out + static_cast<size_t>(KINDS) * row;
         const uint4 to = reinterpret_cast<const uint4*>(args.run_prefix)[end];
         const uint4 from = reinterpret_cast<const uint4*>(args.run_prefix)[start];
         const uint32_t difference[KINDS] = {to.x - from.x, to.y - from.y, to.z - from.z, to.w - from.w};
#pragma unroll
         for (uint32_t k = 0; k < KINDS; ++k) {
            if (difference[k] != 0) {
               atomicAdd(cell + k, difference[k]);
            }
         }
      }
   }
}

/// A thread per sparse key (grid-stride): an ambiguity code, or the missing symbol where it has neither runs nor a plane.
__global__ __launch_bounds__(THREADS) void k_cell_count_sparse(const CellArgs args) {
   for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < args.n_sparse; i += gridDim.x * THREADS) {
      const uint64_t key = args.sparse_keys[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count) {
         correct(args, row, position, static_cast<uint32_t>(key >> 32) & 31u);
      }
   }
}

size_t align256(size_t bytes) {
   return (bytes + 255u) / 256u * 256u;
}

uint32_t blocksOfWords(uint32_t row_words) {
   return row_words / WORDS_PER_BLOCK + (row_words % WORDS_PER_BLOCK != 0 ? 1u : 0u);
}

uint32_t strideBlocks(uint32_t items) {
   return std::min<uint32_t>((items + THREADS - 1u) / THREADS, 4096u);
}

// ---- the readers of a table ------------------------------------------------------------------------------
/// The sum of the kinds of `mask` of a row's four counts: 64 bits, so that four values near 2^32 do not wrap.
__device__ __forceinline__ uint64_t valueOf(const uint4 cell, uint32_t mask) {
   return static_cast<uint64_t>((mask & 1u) != 0 ? cell.x : 0u) + ((mask & 2u) != 0 ? cell.y : 0u) + ((mask & 4u) != 0 ? cell.z : 0u) +
          ((mask & 8u) != 0 ? cell.w : 0u);
}

/// A thread per row of the table, a wave per word of the bitset: one 16-byte load per lane, the wave's ballot of the predicate is
/// the word, stored by its first lane.  A wave whose word is at or past row_words neither loads nor stores; rows at or past
/// sequence_count give 0 whatever their cell holds.
__global__ __launch_bounds__(THREADS) void k_bitset_from_cell_counts(
   const uint4* __restrict__ table, uint32_t row_words, uint32_t sequence_count, uint32_t kinds_mask, uint32_t at_least, uint32_t at_most,
   uint64_t* __restrict__ out
) {
   const size_t row = static_cast<size_t>(blockIdx.x) * THREADS + threadIdx.x;
   const size_t word = row >> 6;  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint64_t value = valueOf(table[row], kinds_mask);
   const bool selected = row < sequence_count && value >= at_least && value <= at_most;
   const uint64_t bits = __ballot(selected);
   if ((threadIdx.x & 63u) == 0) {
      out[word] = bits;
   }
}

/// grid <= MAX_HISTOGRAM_BLOCKS; a wave takes the filter words wave, wave + waves of the grid, ...  A wave whose selected rows all
/// fall into one bin adds their number once.
__global__ __launch_bounds__(THREADS) void k_cell_count_histogram(
   const uint4* __restrict__ table, uint32_t row_words, uint32_t sequence_count, const uint64_t* __restrict__ filter, uint32_t kinds_mask,
   uint32_t bin_width, uint32_t n_bins, unsigned long long* __restrict__ bins
) {
   __shared__ uint32_t s_bins[MAX_BINS];
   for (uint32_t bin = threadIdx.x; bin < n_bins; bin += THREADS) {
      s_bins[bin] = 0;
   }
   __syncthreads();
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK;
   for (uint64_t word = static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6); word < row_words; word += step) {
      const uint64_t bits = filter != nullptr ? filter[word] : ~0ull;
      const uint64_t row = word * 64u + lane;
      const bool selected = ((bits >> lane) & 1ull) != 0 && row < sequence_count;
      uint32_t bin = 0;
      if (selected) {
         bin = static_cast<uint32_t>(min(valueOf(table[row], kinds_mask) / bin_width, static_cast<uint64_t>(n_bins - 1u)));
      }
      const uint64_t chosen = __ballot(selected);
      if (chosen == 0) {
         continue;
      }
      const uint32_t first_bin = __shfl(bin, __ffsll(static_cast<unsigned long long>(chosen)) - 1);
      if (__ballot(selected && bin == first_bin) == chosen) {
         if (lane == 0) {
            atomicAdd(&s_bins[first_bin], static_cast<uint32_t>(__popcll(chosen)));
         }
      } else if (selected) {
         atomicAdd(&s_bins[bin], 1u);
      }
   }
   __syncthreads();
   for (uint32_t bin = threadIdx.x; bin < n_bins; bin += THREADS) {
      const uint32_t count = s_bins[bin];
      if (count != 0) {
         atomicAdd(bins + bin, static_cast<unsigned long long>(count));
      }
   }
}

int checkTable(const char* entry, const void* table_dev, uint32_t row_words, uint32_t sequence_count, uint32_t kinds_mask) {
   if (table_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad arguments");
   }
   if (row_words == 0 || sequence_count == 0 || sequence_count > static_cast<uint64_t>(row_words) * 64u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": the table has no rows, or fewer than sequence_count");
   }
   if (kinds_mask == 0 || kinds_mask >= (1u << KINDS)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": kinds_mask names no kind, or one that does not exist");
   }
   return SILO_GPU_OK;
}

}  // namespace

extern "C" {

int silo_gpu_row_cell_counts(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t* out_dev, void* scratch_dev, void* stream) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_cell_counts: bad arguments");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (!seqstore.finalized || dev.planes == nullptr || dev.row_words == 0 || seqstore.d_reference.get() == nullptr ||
       seqstore.reference.size() != dev.positions) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_cell_counts: store is not finalized");
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);
   const uint32_t P = dev.positions;
   const uint32_t missing = dev.missing_symbol;
   const uint32_t valid = seqstore.alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE ? VALID_NUCLEOTIDES : VALID_AMINO_ACIDS;

   // the per-position tables: what an open cell of the planes counts as, and the running sums a run of the missing symbol reads
   uint8_t symbol_of_scan[SCAN_SLOTS];
   std::fill(symbol_of_scan, symbol_of_scan + SCAN_SLOTS, NO_SCAN_SYMBOL);
   for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {
      if (dev.kind[symbol] == PLANE_SCAN && dev.index[symbol] < SCAN_SLOTS) {
         symbol_of_scan[dev.index[symbol]] = static_cast<uint8_t>(symbol);
      }
   }
   const bool has_map = dev.code_map != nullptr && !seqstore.layout.code_map.empty();
   const size_t base_bytes = align256(P);
   const size_t prefix_bytes = align256((static_cast<size_t>(P) + 1u) * KINDS * sizeof(uint32_t));
   if (base_bytes + prefix_bytes > SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(P)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_cell_counts: scratch layout exceeds its documented size");  // (cannot happen)
   }
   std::vector<uint8_t> tables(base_bytes + prefix_bytes, 0);
   uint8_t* t_base = tables.data();
   auto* t_prefix = reinterpret_cast<uint32_t*>(tables.data() + base_bytes);
   for (uint32_t p = 0; p < P; ++p) {
      uint32_t base = NO_SYMBOL;
      if (has_map) {
         const uint8_t* map = seqstore.layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
         if ((map[0] & LAYOUT_IMPLICIT) != 0 && map[IMPLICIT_SLOT] < SCAN_SLOTS && symbol_of_scan[map[IMPLICIT_SLOT]] != NO_SCAN_SYMBOL) {
            base = symbol_of_scan[map[IMPLICIT_SLOT]];
         }
      }
      t_base[p] = static_cast<uint8_t>(base);
      const uint32_t of_missing = classOf(missing, seqstore.reference[p], missing, valid);
      const uint32_t of_base = classOf(base, seqstore.reference[p], missing, valid);
      for (uint32_t k = 0; k < KINDS; ++k) {
         t_prefix[KINDS * (p + 1u) + k] = t_prefix[KINDS * p + k] + (of_missing == k ? 1u : 0u) - (of_base == k ? 1u : 0u);
      }
   }
   auto* scratch = static_cast<uint8_t*>(scratch_dev);
   HIP_TRY(hipMemcpyAsync(scratch, tables.data(), tables.size(), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   CellArgs args{};
   args.dev = dev;
   args.reference = seqstore.d_reference.get();
   args.base_symbol = scratch;
   args.run_prefix = reinterpret_cast<const uint32_t*>(scratch + base_bytes);
   args.sparse_keys = seqstore.d_sparse.get();
   args.n_sparse = seqstore.d_sparse.get() != nullptr ? static_cast<uint32_t>(seqstore.sparse_sorted.size()) : 0u;
   args.n_escapes = has_map && dev.escapes != nullptr && !seqstore.layout.escape_first.empty() ? seqstore.layout.escape_first.back() : 0u;
   args.sequence_count = store->sequence_count;
   args.valid = valid;
   args.out = out_dev;
   if (dev.extra != nullptr) {
      for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {
         if (dev.kind[symbol] == PLANE_EXTRA && args.n_extra < MAX_EXTRA) {
            args.extra_symbols[args.n_extra++] = static_cast<uint8_t>(symbol);
         }
      }
   }
   k_cell_count_planes<<<blocksOfWords(dev.row_words), THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   if (args.n_escapes != 0) {
      k_cell_count_escapes<<<strideBlocks(args.n_escapes), THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (dev.kind[missing] == PLANE_RUNS && dev.n_missing_runs != 0 && dev.missing_run_keys != nullptr && dev.missing_run_ends != nullptr) {
      k_cell_count_runs<<<strideBlocks(dev.n_missing_runs), THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (args.n_sparse != 0) {
      k_cell_count_sparse<<<strideBlocks(args.n_sparse), THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   return SILO_GPU_OK;
}

int silo_gpu_store_row_cell_counts(silo_gpu_store* store, uint32_t seqstore_id, const uint32_t** out_dev, void* stream) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_row_cell_counts: bad arguments");
   }
   const std::lock_guard<std::mutex> lock(store->mutex);
   SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (!seqstore.finalized) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_row_cell_counts: store is not finalized");
   }
   if (!seqstore.row_cell_counts_ready) {
      HIP_TRY(hipSetDevice(store->device));
      const size_t words = static_cast<size_t>(seqstore.dev.row_words) * 64u * KINDS;
      DeviceArray<uint32_t> counts;
      DeviceArray<uint8_t> scratch;
      HIP_TRY(counts.alloc(std::max<size_t>(words, KINDS)));
      HIP_TRY(scratch.alloc(SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(seqstore.dev.positions)));
      if (const int status = silo_gpu_row_cell_counts(store, seqstore_id, counts.get(), scratch.get(), stream); status != SILO_GPU_OK) {
         (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));  // nothing in flight may outlive the two arrays
         return status;
      }
      HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
      seqstore.d_row_cell_counts = std::move(counts);
      seqstore.row_cell_counts_ready = true;
      store->device_bytes += words * sizeof(uint32_t);
   }
   *out_dev = seqstore.d_row_cell_counts.get();
   return SILO_GPU_OK;
}

int silo_gpu_bitset_from_cell_counts(
   const uint32_t* table_dev, uint32_t row_words, uint32_t sequence_count, uint32_t kinds_mask, uint32_t at_least, uint32_t at_most,
   uint64_t* out_bitset_dev, void* stream
) {
   if (out_bitset_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_from_cell_counts: bad arguments");
   }
   if (const int status = checkTable("silo_gpu_bitset_from_cell_counts", table_dev, row_words, sequence_count, kinds_mask); status != SILO_GPU_OK) {
      return status;
   }
   k_bitset_from_cell_counts<<<blocksOfWords(row_words), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const uint4*>(table_dev), row_words, sequence_count, kinds_mask, at_least, at_most, out_bitset_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_cell_count_histogram(
   const uint32_t* table_dev, uint32_t row_words, uint32_t sequence_count, const uint64_t* filter_dev, uint32_t kinds_mask, uint32_t bin_width,
   uint32_t n_bins, uint64_t* bins_dev, void* stream
) {
   if (bins_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_cell_count_histogram: bad arguments");
   }
   if (const int status = checkTable("silo_gpu_cell_count_histogram", table_dev, row_words, sequence_count, kinds_mask); status != SILO_GPU_OK) {
      return status;
   }
   if (bin_width == 0 || n_bins == 0 || n_bins > MAX_BINS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_cell_count_histogram: bin_width is 0, or n_bins is 0 or above SILO_GPU_MAX_CELL_COUNT_BINS");
   }
   k_cell_count_histogram<<<std::min(blocksOfWords(row_words), MAX_HISTOGRAM_BLOCKS), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const uint4*>(table_dev), row_words, sequence_count, filter_dev, kinds_mask, bin_width, n_bins,
      reinterpret_cast<unsigned long long*>(bins_dev)
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
