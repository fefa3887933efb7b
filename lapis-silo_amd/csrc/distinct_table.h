// distinct_table.h — what the kernels over K20's owner table share (silo_gpu_distinct.hip, silo_gpu_distinct_counts.hip): the hash of a
// global row, the load of an owner while other lanes claim slots, the read-only probe to a row's class, and what every entry that
// walks a part's rows refuses.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "store_internal.h"

namespace silo_gpu_distinct_table {

constexpr uint32_t EMPTY = SILO_GPU_DISTINCT_EMPTY;
constexpr uint32_t THREADS = 256;  // four waves: four neighbouring row words per block
constexpr uint32_t WORDS_PER_BLOCK = THREADS / 64u;
constexpr uint32_t MAX_WALK_BLOCKS = 4096;  // of the kernels whose waves stride over the filter words
static_assert(sizeof(silo_gpu_distinct_part) == 24);

/// The hash of global row `g`: the part is the last one whose first_row is <= g.
__device__ __forceinline__ ulonglong2 hashOfGlobalRow(const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, uint32_t g) {
   uint32_t lo = 0, hi = n_parts;
   while (lo < hi) {  // first part whose first_row is beyond g
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (parts[mid].first_row <= g) {
         lo = mid + 1u;
      } else {
         hi = mid;
      }
   }
   const silo_gpu_distinct_part& part = parts[lo != 0 ? lo - 1u : 0u];
   const uint32_t row = g - part.first_row;
   if (row >= part.sequence_count) {  // (no inserted row: cannot be an owner)
      return make_ulonglong2(0ull, 0ull);
   }
   return reinterpret_cast<const ulonglong2*>(part.hashes_dev)[row];
}

__device__ __forceinline__ uint32_t loadOwner(const uint32_t* slot) {
   return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/// The slot of the class of global row `g` with hash `hash` in a table that no launch writes any more — the read-only probe of
/// k_distinct_select: it ends where the owner is the row itself (`is_owner`) or the owner's hash equals the row's.  EMPTY when the
/// probe meets an empty slot or has passed every slot: a row that was never inserted.
__device__ __forceinline__ uint32_t slotOfClass(
   const uint32_t* __restrict__ table, uint32_t slots, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, uint32_t g, ulonglong2 hash,
   bool& is_owner
) {
   const uint32_t mask = slots - 1u;
   uint32_t slot = static_cast<uint32_t>(hash.x) & mask;
   is_owner = false;
   for (uint32_t probes = 0; probes < slots; ++probes) {
      const uint32_t owner = table[slot];
      if (owner == EMPTY) {
         return EMPTY;
      }
      if (owner == g) {
         is_owner = true;
         return slot;
      }
      const ulonglong2 other = hashOfGlobalRow(parts, n_parts, owner);
      if (other.x == hash.x && other.y == hash.y) {
         return slot;
      }
      slot = (slot + 1u) & mask;
   }
   return EMPTY;
}

/// What the entries that walk a part's rows refuse; reads parts_dev[part] back into `mine`.
inline int checkSelection(
   const char* what, const void* table, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part, const void* filter,
   const void* out, hipStream_t hip_stream, silo_gpu_distinct_part& mine
) {
   using silo_gpu_detail::fail;
   if (table == nullptr || parts_dev == nullptr || filter == nullptr || out == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": bad arguments");
   }
   if (slots == 0 || (slots & (slots - 1u)) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": slots has to be a power of two");
   }
   if (n_parts == 0 || part >= n_parts) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": no parts, or a part past the last one");
   }
   HIP_TRY(hipMemcpyAsync(&mine, parts_dev + part, sizeof(mine), hipMemcpyDeviceToHost, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));
   if (mine.hashes_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": the part has no hashes");
   }
   if (mine.row_words == 0 || mine.sequence_count > static_cast<uint64_t>(mine.row_words) * 64u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": no row words, or fewer rows than sequence_count");
   }
   if (static_cast<uint64_t>(mine.first_row) + mine.sequence_count >= 0xFFFFFFFFull) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": first_row + sequence_count has to stay below 2^32 - 1");
   }
   return SILO_GPU_OK;
}

}  // namespace silo_gpu_distinct_table
