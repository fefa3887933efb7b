// silo_gpu_cell_counts.hip — K22, the filter expression CellCount and the action CellCountDistribution: per row of a
// sequence store the number of its cells that are a substitution, a deletion, the missing symbol or ambiguous against the store's
// own reference — K18's four cell counts (silo_gpu_differences.hip), over all positions — kept by the store; a row bitset from a
// bound on the sum of some of the four; and the histogram of that sum over the selected rows.
// The counts are read off the store's layout by the pass of row_fold.h, which decides what symbol a cell holds; CellCountFold says
// what the symbol is worth — a class vector: one of the four counts is 1, or none for a cell that equals the reference — mod 2^32:
//   k_cell_count_planes     foldPlanes: the four sums stay in registers and leave with one 16-byte store per row (zeros for padding rows)
//   k_cell_count_escapes    foldEscapes: class(its symbol) - class(what the planes said) per escape key, at most one -1 and one +1
//   k_cell_count_runs       foldRuns: two lookups in a prefix array of those differences per run of the missing symbol
//   k_cell_count_sparse     foldSparse: the same difference per sparse key (ambiguity code)
// The two readers of such a table take no store:
//   k_bitset_from_cell_counts  a thread per row, a wave's ballot per word
//   k_cell_count_histogram     a wave per filter word, a lane per selected row; a block's bins in LDS, flushed with 64-bit adds
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <string>

#include "cell_class.h"
#include "row_fold.h"
#include "store_internal.h"

using namespace silo_gpu_detail;
using namespace silo_gpu_row_fold;
using namespace silo_gpu_cell_class;

namespace {

constexpr uint32_t THREADS = 256;  // four waves: four neighbouring row words per block
constexpr uint32_t WORDS_PER_BLOCK = THREADS / 64u;
constexpr uint32_t KINDS = SILO_GPU_CELL_COUNT_KINDS;
constexpr uint32_t MAX_BINS = SILO_GPU_MAX_CELL_COUNT_BINS;
constexpr uint32_t MAX_HISTOGRAM_BLOCKS = 2048;
static_assert(KINDS == SILO_GPU_DIFFERENCE_STATS && KINDS == 4);

/// The policy of the layout pass (row_fold.h): a row's value is the sum of its cells' class vectors, mod 2^32 in each of the four.
struct CellCountFold {
   using Value = uint4;
   const uint8_t* reference;  // [P] symbol indices
   uint32_t valid;            // the alphabet's valid mutation symbols, a bit per symbol index
   uint32_t missing;          // the store's missing symbol
   const Value* run_prefix;   // [P + 1] sums over q < p of class(q, missing symbol) - class(q, base_symbol[q])
   Value* out;                // [row_words * 64]

   __device__ static Value zero() { return make_uint4(0u, 0u, 0u, 0u); }
   __device__ void add(Value& value, uint32_t position, uint32_t symbol) const {
      const uint32_t cell_class = classOf(symbol, reference[position], missing, valid);
      value.x += cell_class == SUBSTITUTION ? 1u : 0u;
      value.y += cell_class == DELETION ? 1u : 0u;
      value.z += cell_class == MISSING ? 1u : 0u;
      value.w += cell_class == AMBIGUOUS ? 1u : 0u;
   }
   __device__ void store(uint64_t row, Value value) const { out[row] = value; }
   /// Adds class(position, symbol) - class(position, base) to the row's cell: at most one +1 and one -1.
   __device__ void correct(uint32_t row, uint32_t position, uint32_t symbol, uint32_t base) const {
      const uint32_t now = classOf(symbol, reference[position], missing, valid);
      const uint32_t before = classOf(base, reference[position], missing, valid);
      if (now == before) {
         return;
      }
      uint32_t* cell = reinterpret_cast<uint32_t*>(out + row);
      if (now != SAME) {
         atomicAdd(cell + now, 1u);
      }
      if (before != SAME) {
         atomicAdd(cell + before, 0xFFFFFFFFu);
      }
   }
   __device__ void correctRun(uint32_t row, uint32_t start, uint32_t end) const {
      uint32_t* cell = reinterpret_cast<uint32_t*>(out + row);
      const Value to = run_prefix[end];
      const Value from = run_prefix[start];
      const uint32_t difference[KINDS] = {to.x - from.x, to.y - from.y, to.z - from.z, to.w - from.w};
#pragma unroll
      for (uint32_t k = 0; k < KINDS; ++k) {
         if (difference[k] != 0) {
            atomicAdd(cell + k, difference[k]);
         }
      }
   }
   Value nextPrefix(Value previous, uint32_t position, uint32_t base, const SeqStoreHost& seqstore) const {
      const uint32_t of_missing = classOf(missing, seqstore.reference[position], missing, valid);
      const uint32_t of_base = classOf(base, seqstore.reference[position], missing, valid);
      const auto step = [&](uint32_t sum, uint32_t k) { return sum + (of_missing == k ? 1u : 0u) - (of_base == k ? 1u : 0u); };
      return make_uint4(step(previous.x, SUBSTITUTION), step(previous.y, DELETION), step(previous.z, MISSING), step(previous.w, AMBIGUOUS));
   }
};

__global__ __launch_bounds__(FOLD_THREADS) void k_cell_count_planes(const LayoutArgs args, const CellCountFold fold) {
   foldPlanes(args, fold);
}
__global__ __launch_bounds__(FOLD_THREADS) void k_cell_count_escapes(const LayoutArgs args, const CellCountFold fold) {
   foldEscapes(args, fold);
}
__global__ __launch_bounds__(FOLD_THREADS) void k_cell_count_runs(const LayoutArgs args, const CellCountFold fold) {
   foldRuns(args, fold);
}
__global__ __launch_bounds__(FOLD_THREADS) void k_cell_count_sparse(const LayoutArgs args, const CellCountFold fold) {
   foldSparse(args, fold);
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
   const uint32_t valid = seqstore.alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE ? VALID_NUCLEOTIDES : VALID_AMINO_ACIDS;
   return foldRows(
      "silo_gpu_row_cell_counts", store, seqstore, scratch_dev, SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(dev.positions), static_cast<hipStream_t>(stream),
      CellCountFold{seqstore.d_reference.get(), valid, dev.missing_symbol, nullptr, reinterpret_cast<uint4*>(out_dev)},
      {k_cell_count_planes, k_cell_count_escapes, k_cell_count_runs, k_cell_count_sparse}
   );
}

int silo_gpu_store_row_cell_counts(silo_gpu_store* store, uint32_t seqstore_id, const uint32_t** out_dev, void* stream) {
   return keptRowTable<uint32_t>(
      "silo_gpu_store_row_cell_counts", store, seqstore_id, out_dev, stream, &SeqStoreHost::d_row_cell_counts, &SeqStoreHost::row_cell_counts_ready,
      [](uint32_t positions) -> size_t { return SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(positions); }, silo_gpu_row_cell_counts
   );
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
   k_bitset_from_cell_counts<<<blocksOfWords(row_words, WORDS_PER_BLOCK), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
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
   k_cell_count_histogram<<<std::min(blocksOfWords(row_words, WORDS_PER_BLOCK), MAX_HISTOGRAM_BLOCKS), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const uint4*>(table_dev), row_words, sequence_count, filter_dev, kinds_mask, bin_width, n_bins,
      reinterpret_cast<unsigned long long*>(bins_dev)
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
