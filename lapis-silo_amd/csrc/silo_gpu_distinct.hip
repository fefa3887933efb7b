// silo_gpu_distinct.hip — K20, the filter expression DistinctSequences: a 128-bit hash of every row of a sequence
// store (row_hash.h), kept by the store, and a hash-table pass over the selected rows of any number of partitions that leaves one
// row — the one with the smallest number in the database — per class of rows with equal hashes.
// The hashes are read off the store's layout by the pass of row_fold.h, which decides what symbol a cell holds; RowHashFold says
// what the symbol is worth — every row gets the terms of what the planes say, and each stored thing beside the planes corrects its
// cell with the difference of two terms, mod 2^64:
//   k_row_hash_planes    foldPlanes: the two sums stay in registers and leave with one 16-byte store per row ((0, 0) for padding rows)
//   k_row_hash_escapes   foldEscapes: H(p, its symbol) - H(p, what the planes said) per escape key
//   k_row_hash_runs      foldRuns: two lookups in a prefix array of those differences per run of the missing symbol
//   k_row_hash_sparse    foldSparse: the same difference per sparse key (ambiguity code)
// The selection, on row bitsets and arrays of hashes, takes no store (what it shares with the class counts of K21 — the hash of a
// global row, the load of an owner, the refusals — is in distinct_table.h):
//   k_distinct_begin     every slot of the owner table empty, the overflow counter 0
//   k_distinct_insert    a wave per filter word, a lane per selected row: linear probing with compare-and-swap / atomic min
//   k_distinct_select    a thread per row, a wave's ballot per word: the rows that own their class's slot
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <string>

#include "distinct_table.h"
#include "row_fold.h"
#include "row_hash.h"
#include "store_internal.h"

using namespace silo_gpu_detail;
using namespace silo_gpu_distinct_table;
using namespace silo_gpu_row_fold;
using silo_gpu_row_hash::term;

namespace {

static_assert(silo_gpu_row_hash::NO_SYMBOL == NO_SYMBOL);

/// The policy of the layout pass (row_fold.h): a row's value is the sum of its cells' terms, mod 2^64 in each of the two lanes.
struct RowHashFold {
   using Value = ulonglong2;
   const Value* run_prefix;  // [P + 1] sums over q < p of H(q, missing symbol) - H(q, base_symbol[q])
   Value* out;               // [row_words * 64]

   __device__ static Value zero() { return make_ulonglong2(0ull, 0ull); }
   __device__ void add(Value& value, uint32_t position, uint32_t symbol) const {
      value.x += term(position, symbol, 0);
      value.y += term(position, symbol, 1);
   }
   __device__ void store(uint64_t row, Value value) const { out[row] = value; }
   /// Adds H(position, symbol) - H(position, base) to the row's cell, lane by lane.
   __device__ void correct(uint32_t row, uint32_t position, uint32_t symbol, uint32_t base) const {
      if (symbol == base) {
         return;
      }
      auto* cell = reinterpret_cast<unsigned long long*>(out + row);
      atomicAdd(cell, static_cast<unsigned long long>(term(position, symbol, 0) - term(position, base, 0)));
      atomicAdd(cell + 1, static_cast<unsigned long long>(term(position, symbol, 1) - term(position, base, 1)));
   }
   __device__ void correctRun(uint32_t row, uint32_t start, uint32_t end) const {
      auto* cell = reinterpret_cast<unsigned long long*>(out + row);
      const Value to = run_prefix[end];
      const Value from = run_prefix[start];
      atomicAdd(cell, static_cast<unsigned long long>(to.x - from.x));
      atomicAdd(cell + 1, static_cast<unsigned long long>(to.y - from.y));
   }
   Value nextPrefix(Value previous, uint32_t position, uint32_t base, const SeqStoreHost& seqstore) const {
      const uint32_t missing = seqstore.dev.missing_symbol;
      return make_ulonglong2(
         previous.x + (term(position, missing, 0) - term(position, base, 0)), previous.y + (term(position, missing, 1) - term(position, base, 1))
      );
   }
};

__global__ __launch_bounds__(FOLD_THREADS) void k_row_hash_planes(const LayoutArgs args, const RowHashFold fold) {
   foldPlanes(args, fold);
}
__global__ __launch_bounds__(FOLD_THREADS) void k_row_hash_escapes(const LayoutArgs args, const RowHashFold fold) {
   foldEscapes(args, fold);
}
__global__ __launch_bounds__(FOLD_THREADS) void k_row_hash_runs(const LayoutArgs args, const RowHashFold fold) {
   foldRuns(args, fold);
}
__global__ __launch_bounds__(FOLD_THREADS) void k_row_hash_sparse(const LayoutArgs args, const RowHashFold fold) {
   foldSparse(args, fold);
}

// ---- the selection ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_distinct_begin(uint32_t* __restrict__ table, uint32_t slots) {
   const uint64_t word = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
   if (word <= slots) {
      table[word] = word == slots ? 0u : EMPTY;  // the overflow counter sits behind the slots
   }
}

/// grid <= MAX_WALK_BLOCKS; a wave takes the filter words wave, wave + waves of the grid, ...  No lane waits for another: every
/// step of the probe is one atomic whose outcome is final for that slot's class.
__global__ __launch_bounds__(THREADS) void k_distinct_insert(
   uint32_t* __restrict__ table, uint32_t slots, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, uint32_t part,
   const uint64_t* __restrict__ filter
) {
   const silo_gpu_distinct_part mine = parts[part];
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t mask = slots - 1u;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK;
   for (uint64_t word = static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6); word < mine.row_words; word += step) {
      const uint64_t bits = filter[word];
      const uint64_t row = word * 64u + lane;
      if (((bits >> lane) & 1ull) == 0 || row >= mine.sequence_count) {
         continue;
      }
      const ulonglong2 hash = reinterpret_cast<const ulonglong2*>(mine.hashes_dev)[row];
      const uint32_t g = mine.first_row + static_cast<uint32_t>(row);
      uint32_t slot = static_cast<uint32_t>(hash.x) & mask;
      bool placed = false;
      for (uint32_t probes = 0; probes < slots && !placed; ++probes) {
         uint32_t owner = loadOwner(table + slot);
         if (owner == EMPTY) {
            owner = atomicCAS(table + slot, EMPTY, g);
            if (owner == EMPTY) {
               placed = true;
               break;
            }
         }
         if (owner == g) {
            placed = true;
            break;
         }
         const ulonglong2 other = hashOfGlobalRow(parts, n_parts, owner);
         if (other.x == hash.x && other.y == hash.y) {
            if (g < owner) {
               atomicMin(table + slot, g);
            }
            placed = true;
            break;
         }
         slot = (slot + 1u) & mask;
      }
      if (!placed) {
         atomicAdd(table + slots, 1u);
      }
   }
}

/// A thread per row, a wave per word of the output: a wave whose word is at or past row_words neither loads nor stores.
__global__ __launch_bounds__(THREADS) void k_distinct_select(
   const uint32_t* __restrict__ table, uint32_t slots, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, uint32_t part,
   const uint64_t* __restrict__ filter, uint64_t* __restrict__ out
) {
   const silo_gpu_distinct_part mine = parts[part];
   const uint64_t row = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
   const uint64_t word = row >> 6;  // (uniform over the wave)
   if (word >= mine.row_words) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t bits = filter[word];
   bool selected = false;
   if (((bits >> lane) & 1ull) != 0 && row < mine.sequence_count) {
      const ulonglong2 hash = reinterpret_cast<const ulonglong2*>(mine.hashes_dev)[row];
      const uint32_t g = mine.first_row + static_cast<uint32_t>(row);
      (void)slotOfClass(table, slots, parts, n_parts, g, hash, selected);  // the row owns its class's slot
   }
   const uint64_t ballot = __ballot(selected);
   if (lane == 0) {
      out[word] = ballot;
   }
}

}  // namespace

extern "C" {

uint64_t silo_gpu_row_hash_term(uint32_t position, uint32_t symbol, uint32_t lane) {
   return term(position, symbol, lane != 0 ? 1u : 0u);
}

int silo_gpu_row_hashes(const silo_gpu_store* store, uint32_t seqstore_id, uint64_t* out_dev, void* scratch_dev, void* stream) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_hashes: bad arguments");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (!seqstore.finalized || dev.planes == nullptr || dev.row_words == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_hashes: store is not finalized");
   }
   return foldRows(
      "silo_gpu_row_hashes", store, seqstore, scratch_dev, SILO_GPU_ROW_HASH_SCRATCH_BYTES(dev.positions), static_cast<hipStream_t>(stream),
      RowHashFold{nullptr, reinterpret_cast<ulonglong2*>(out_dev)}, {k_row_hash_planes, k_row_hash_escapes, k_row_hash_runs, k_row_hash_sparse}
   );
}

int silo_gpu_store_row_hashes(silo_gpu_store* store, uint32_t seqstore_id, const uint64_t** out_dev, void* stream) {
   return keptRowTable<uint64_t>(
      "silo_gpu_store_row_hashes", store, seqstore_id, out_dev, stream, &SeqStoreHost::d_row_hashes, &SeqStoreHost::row_hashes_ready,
      [](uint32_t positions) -> size_t { return SILO_GPU_ROW_HASH_SCRATCH_BYTES(positions); }, silo_gpu_row_hashes
   );
}

int silo_gpu_distinct_begin(void* table_dev, uint32_t slots, void* stream) {
   if (table_dev == nullptr || slots == 0 || (slots & (slots - 1u)) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_distinct_begin: no table, or slots is not a power of two");
   }
   const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(slots) + 1u + THREADS - 1u) / THREADS);
   k_distinct_begin<<<blocks, THREADS, 0, static_cast<hipStream_t>(stream)>>>(static_cast<uint32_t*>(table_dev), slots);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distinct_insert(
   void* table_dev, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part, const uint64_t* filter_dev,
   void* stream
) {
   auto hip_stream = static_cast<hipStream_t>(stream);
   silo_gpu_distinct_part mine{};
   if (const int status = checkSelection("silo_gpu_distinct_insert", table_dev, slots, parts_dev, n_parts, part, filter_dev, table_dev, hip_stream, mine);
       status != SILO_GPU_OK) {
      return status;
   }
   k_distinct_insert<<<std::min(blocksOfWords(mine.row_words, WORDS_PER_BLOCK), MAX_WALK_BLOCKS), THREADS, 0, hip_stream>>>(
      static_cast<uint32_t*>(table_dev), slots, parts_dev, n_parts, part, filter_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distinct_select(
   const void* table_dev, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, uint64_t* out_bitset_dev, void* stream
) {
   auto hip_stream = static_cast<hipStream_t>(stream);
   silo_gpu_distinct_part mine{};
   if (const int status = checkSelection("silo_gpu_distinct_select", table_dev, slots, parts_dev, n_parts, part, filter_dev, out_bitset_dev, hip_stream, mine);
       status != SILO_GPU_OK) {
      return status;
   }
   k_distinct_select<<<blocksOfWords(mine.row_words, WORDS_PER_BLOCK), THREADS, 0, hip_stream>>>(
      static_cast<const uint32_t*>(table_dev), slots, parts_dev, n_parts, part, filter_dev, out_bitset_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
