// silo_gpu_distinct_counts.hip — K21, the action DistinctSequenceCounts: the sizes of the classes of K20's owner table
// and the largest of them, all on the device.  On a table that every part's silo_gpu_distinct_insert has filled (distinct_table.h):
//   k_distinct_count     a wave per filter word, a lane per selected row: the read-only probe to the slot of the row's class, then
//                        one atomic add per distinct slot among the wave's lanes (a leader's slot, a ballot of its peers)
//   k_distinct_classes   the same walk, 16 words at a time: a row that owns its slot and whose class is large enough appends the key
//                        (0xFFFFFFFF - count) << 32 | global row; one atomic add on the key counter per wave and step
// and, on any list of pairwise distinct 64-bit keys whose length is known to the device only, the k smallest by a radix select in
// K19's pattern (silo_gpu_sample.hip) — one group, eight rounds of 8 bits, most significant first:
//   k_keys_histogram     grid-stride over the keys that continue the prefix: a block's 256 cells in LDS, its non-zero cells added
//                        to the table
//   k_keys_advance       one block: running sums of the 256 cells, the digit where they reach the keys still to take; clears them
//   k_keys_gather        a wave-aggregated append of every key <= the threshold (every key, when there are no more than k)
// Nothing returns to the host between the launches, stream order is the only synchronisation between them, and every sum is one of
// integers: no result depends on how the blocks are scheduled.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <string>

#include "distinct_table.h"
#include "store_internal.h"

using namespace silo_gpu_detail;
using namespace silo_gpu_distinct_table;

namespace {

// How many leaders a wave of k_distinct_count serves before its remaining lanes add 1 each.  Rows lie in lineage and date order, so
// the copies of a sequence are mostly neighbours and a word of 64 rows holds few classes of more than one row; a wave that still has
// lanes left after 8 leaders is taken for one whose rows are mostly alone in their classes, where a further round retires one lane
// and costs as much as the add it saves.  Chosen by that argument, NOT measured; the counts do not depend on it.
constexpr uint32_t LEADER_ROUNDS = 8;

constexpr uint32_t CLASS_WORDS = 16;  // filter words (1 024 rows) a wave of k_distinct_classes takes per add on the key counter

constexpr uint32_t DIGITS = 256;          // 8 key bits per round
constexpr uint32_t KEY_ROUNDS = 8;        // of a 64-bit key
constexpr uint32_t MAX_KEY_BLOCKS = 1024;  // of k_keys_histogram and k_keys_gather: four per compute unit
static_assert(THREADS == DIGITS);  // k_keys_advance: a thread per cell

// the scratch of silo_gpu_smallest_keys as uint32 words: the histogram, then the state
enum ScratchWord : uint32_t { TAKE_ALL = DIGITS, REMAINING = DIGITS + 1, APPENDED = DIGITS + 2, PREFIX = DIGITS + 4 /* 64 bits, 8-byte aligned */, SCRATCH_WORDS = DIGITS + 6 };
static_assert(SCRATCH_WORDS * sizeof(uint32_t) <= SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES && (PREFIX * sizeof(uint32_t)) % 8 == 0);

/// Row `lane` of filter word `word` of the part, when it counts: its slot in the table (EMPTY for a row that does not count, and for
/// one that counts but was never inserted, which adds 1 to the overflow counter behind the slots).
__device__ __forceinline__ uint32_t slotOfLane(
   uint32_t* __restrict__ table, uint32_t slots, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, const silo_gpu_distinct_part& mine,
   uint64_t bits, uint64_t word, uint32_t lane, uint32_t& g, bool& is_owner
) {
   const uint64_t row = word * 64u + lane;
   is_owner = false;
   if (((bits >> lane) & 1ull) == 0 || row >= mine.sequence_count) {
      return EMPTY;
   }
   const ulonglong2 hash = reinterpret_cast<const ulonglong2*>(mine.hashes_dev)[row];
   g = mine.first_row + static_cast<uint32_t>(row);
   const uint32_t slot = slotOfClass(table, slots, parts, n_parts, g, hash, is_owner);
   if (slot == EMPTY) {  // (cannot occur after the inserts of every part)
      atomicAdd(table + slots, 1u);
   }
   return slot;
}

/// grid <= MAX_WALK_BLOCKS; a wave takes the filter words wave, wave + waves of the grid, ... (k_distinct_insert's shape).  The table is
/// only read here (but for the overflow counter); counts takes integer adds only.
__global__ __launch_bounds__(THREADS) void k_distinct_count(
   uint32_t* __restrict__ table, uint32_t slots, uint32_t* __restrict__ counts, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts,
   uint32_t part, const uint64_t* __restrict__ filter
) {
   const silo_gpu_distinct_part mine = parts[part];
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK;
   for (uint64_t word = static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6); word < mine.row_words; word += step) {
      const uint64_t bits = filter[word];  // (uniform over the wave, as is the loop)
      if (bits == 0) {
         continue;
      }
      uint32_t g = 0;
      bool is_owner = false;
      const uint32_t slot = slotOfLane(table, slots, parts, n_parts, mine, bits, word, lane, g, is_owner);
      bool pending = slot != EMPTY;
      // one add per distinct slot among the lanes: the first pending lane's slot leads, the lanes that share it retire together
      for (uint32_t round = 0; round < LEADER_ROUNDS && __ballot(pending) != 0; ++round) {
         if (pending) {
            const uint32_t leader = __builtin_amdgcn_readfirstlane(slot);
            const bool peer = slot == leader;
            const uint64_t peers = __ballot(peer);  // (of the pending lanes: the others are not active here)
            if (peer) {
               if (lane == static_cast<uint32_t>(__ffsll(static_cast<long long>(peers))) - 1u) {
                  atomicAdd(counts + leader, static_cast<uint32_t>(__popcll(peers)));
               }
               pending = false;
            }
         }
      }
      if (pending) {
         atomicAdd(counts + slot, 1u);
      }
   }
}

/// grid <= MAX_WALK_BLOCKS; a wave takes CLASS_WORDS neighbouring filter words at a time — with the walk and the probe of
/// k_distinct_count — and keeps each lane's class size of every one of them (0: the lane appends nothing); then ONE atomic add on
/// *n_keys reserves room for all the keys of the step, and a lane's place is the ballots' popcount of the words and lanes before
/// it.  (One add per word is one returning atomic on one address per 64 rows: measured on 10 M rows, it alone took 1.9 ms.)
/// *n_keys counts every class that qualifies; a key whose index is at or past `capacity` is not written.
__global__ __launch_bounds__(THREADS) void k_distinct_classes(
   uint32_t* __restrict__ table, uint32_t slots, const uint32_t* __restrict__ counts, const silo_gpu_distinct_part* __restrict__ parts,
   uint32_t n_parts, uint32_t part, const uint64_t* __restrict__ filter, uint32_t min_count, uint64_t* __restrict__ keys, uint32_t capacity,
   uint32_t* __restrict__ n_keys
) {
   const silo_gpu_distinct_part mine = parts[part];
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t below = (1ull << lane) - 1ull;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK * CLASS_WORDS;
   for (uint64_t first = (static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6)) * CLASS_WORDS; first < mine.row_words; first += step) {
      uint32_t size[CLASS_WORDS];  // (the loop and everything indexed by w are uniform over the wave)
      uint64_t emitters[CLASS_WORDS];
      uint32_t total = 0;
#pragma unroll
      for (uint32_t w = 0; w < CLASS_WORDS; ++w) {
         const uint64_t word = first + w;
         const uint64_t bits = word < mine.row_words ? filter[word] : 0ull;
         size[w] = 0;
         if (bits != 0) {
            uint32_t g = 0;
            bool is_owner = false;
            const uint32_t slot = slotOfLane(table, slots, parts, n_parts, mine, bits, word, lane, g, is_owner);
            if (slot != EMPTY && is_owner) {
               const uint32_t count = counts[slot];
               size[w] = count >= min_count ? count : 0u;
            }
         }
         emitters[w] = __ballot(size[w] != 0);
         total += static_cast<uint32_t>(__popcll(emitters[w]));
      }
      if (total == 0) {
         continue;
      }
      uint32_t base = 0;
      if (lane == 0) {
         base = atomicAdd(n_keys, total);
      }
      uint64_t index = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(base));
#pragma unroll
      for (uint32_t w = 0; w < CLASS_WORDS; ++w) {
         const uint64_t mine_at = index + static_cast<uint32_t>(__popcll(emitters[w] & below));
         if (size[w] != 0 && mine_at < capacity) {
            const uint32_t g = mine.first_row + static_cast<uint32_t>((first + w) * 64u + lane);
            keys[mine_at] = (static_cast<uint64_t>(0xFFFFFFFFu - size[w]) << 32) | g;
         }
         index += static_cast<uint32_t>(__popcll(emitters[w]));
      }
   }
}

// ---- the k smallest keys ---------------------------------------------------------------------------------
/// How many keys the list holds: what the device counted, but no more than the list has room for.
__device__ __forceinline__ uint32_t keysInList(const uint32_t* __restrict__ n_keys, uint32_t capacity) {
   return min(*n_keys, capacity);
}

/// grid <= MAX_KEY_BLOCKS, sized from the capacity: a block whose first key is past the list leaves at once.  Round r counts the
/// digit (bits 56 - 8r .. 63 - 8r) of every key whose 8r bits above it equal the prefix.
__global__ __launch_bounds__(THREADS) void k_keys_histogram(
   const uint64_t* __restrict__ keys, const uint32_t* __restrict__ n_keys, uint32_t capacity, uint32_t* __restrict__ scratch, uint32_t round
) {
   __shared__ uint32_t s_hist[DIGITS];
   const uint32_t n = keysInList(n_keys, capacity);
   if (static_cast<uint64_t>(blockIdx.x) * THREADS >= n || scratch[TAKE_ALL] != 0) {  // (uniform over the block)
      return;
   }
   s_hist[threadIdx.x] = 0;
   __syncthreads();
   const uint64_t prefix = *reinterpret_cast<const uint64_t*>(scratch + PREFIX);
   const uint32_t shift = 56u - 8u * round;
   for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * THREADS) {
      const uint64_t key = keys[i];
      if (round == 0 || (key >> (shift + 8u)) == prefix) {
         atomicAdd(&s_hist[static_cast<uint32_t>(key >> shift) & 0xFFu], 1u);
      }
   }
   __syncthreads();
   const uint32_t count = s_hist[threadIdx.x];
   if (count != 0) {
      atomicAdd(&scratch[threadIdx.x], count);
   }
}

/// One block, thread d owns cell d.  Round 0 finds a list of no more than k keys (take-all) and otherwise begins with k keys to take;
/// every round appends the digit at which the running sums reach the keys still to take and subtracts the cells in front of it.
/// After round 7 the prefix is the k-th smallest key (the keys are pairwise distinct), and *out_count = min(n, k) is written.
__global__ __launch_bounds__(THREADS) void k_keys_advance(
   const uint32_t* __restrict__ n_keys, uint32_t capacity, uint32_t k, uint32_t* __restrict__ scratch, uint32_t round, uint32_t* __restrict__ out_count
) {
   __shared__ uint32_t s_sum[DIGITS];
   const uint32_t n = keysInList(n_keys, capacity);
   const uint32_t count = scratch[threadIdx.x];
   scratch[threadIdx.x] = 0;
   const uint32_t remaining = round == 0 ? k : scratch[REMAINING];
   const uint64_t prefix = round == 0 ? 0ull : *reinterpret_cast<const uint64_t*>(scratch + PREFIX);
   const bool take_all = round == 0 ? n <= k : scratch[TAKE_ALL] != 0;  // (uniform over the block)
   __syncthreads();  // every thread has read the state before one of them writes it
   if (round + 1u == KEY_ROUNDS && threadIdx.x == 0) {
      *out_count = min(n, k);
   }
   if (take_all) {
      if (round == 0 && threadIdx.x == 0) {
         scratch[TAKE_ALL] = 1;
      }
      return;
   }
   s_sum[threadIdx.x] = count;
   __syncthreads();
   for (uint32_t offset = 1; offset < DIGITS; offset <<= 1) {  // inclusive running sums
      const uint32_t before = threadIdx.x >= offset ? s_sum[threadIdx.x - offset] : 0u;
      __syncthreads();
      s_sum[threadIdx.x] += before;
      __syncthreads();
   }
   const uint32_t upto = s_sum[threadIdx.x];
   const uint32_t before = upto - count;
   if (before < remaining && upto >= remaining) {  // one thread: the cells sum to at least the keys still to take
      *reinterpret_cast<uint64_t*>(scratch + PREFIX) = (prefix << 8) | threadIdx.x;
      scratch[REMAINING] = remaining - before;
   }
}

/// grid <= MAX_KEY_BLOCKS; a wave takes 64 neighbouring keys at a time.  One atomic add on the append counter per wave and step; a
/// key whose index is at or past k (keys equal to the threshold: the caller's keys were not distinct) is not written.
__global__ __launch_bounds__(THREADS) void k_keys_gather(
   const uint64_t* __restrict__ keys, const uint32_t* __restrict__ n_keys, uint32_t capacity, uint32_t k, uint32_t* __restrict__ scratch,
   uint64_t* __restrict__ out
) {
   const uint32_t n = keysInList(n_keys, capacity);
   const bool take_all = scratch[TAKE_ALL] != 0;
   const uint64_t threshold = *reinterpret_cast<const uint64_t*>(scratch + PREFIX);
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * THREADS;
   for (uint64_t first = static_cast<uint64_t>(blockIdx.x) * THREADS + (threadIdx.x & ~63u); first < n; first += step) {  // (uniform over the wave)
      const uint64_t i = first + lane;
      uint64_t key = 0;
      bool taken = false;
      if (i < n) {
         key = keys[i];
         taken = take_all || key <= threshold;
      }
      const uint64_t takers = __ballot(taken);
      if (takers == 0) {
         continue;
      }
      uint32_t base = 0;
      if (lane == static_cast<uint32_t>(__ffsll(static_cast<long long>(takers))) - 1u) {
         base = atomicAdd(&scratch[APPENDED], static_cast<uint32_t>(__popcll(takers)));
      }
      base = __shfl(base, __ffsll(static_cast<long long>(takers)) - 1);
      const uint64_t index = static_cast<uint64_t>(base) + static_cast<uint32_t>(__popcll(takers & ((1ull << lane) - 1ull)));
      if (taken && index < k) {
         out[index] = key;
      }
   }
}

uint32_t walkBlocks(uint32_t row_words) {
   return std::min(blocksOfWords(row_words, WORDS_PER_BLOCK), MAX_WALK_BLOCKS);
}

}  // namespace

extern "C" {

int silo_gpu_distinct_count(
   void* table_dev, uint32_t slots, uint32_t* counts_dev, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, void* stream
) {
   auto hip_stream = static_cast<hipStream_t>(stream);
   silo_gpu_distinct_part mine{};
   if (const int status = checkSelection("silo_gpu_distinct_count", table_dev, slots, parts_dev, n_parts, part, filter_dev, counts_dev, hip_stream, mine);
       status != SILO_GPU_OK) {
      return status;
   }
   k_distinct_count<<<walkBlocks(mine.row_words), THREADS, 0, hip_stream>>>(
      static_cast<uint32_t*>(table_dev), slots, counts_dev, parts_dev, n_parts, part, filter_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distinct_classes(
   void* table_dev, uint32_t slots, const uint32_t* counts_dev, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, uint32_t min_count, uint64_t* keys_dev, uint32_t capacity, uint32_t* n_keys_dev, void* stream
) {
   if (counts_dev == nullptr || n_keys_dev == nullptr || capacity == 0 || min_count == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_distinct_classes: no counts or key counter, a capacity of 0, or a min_count of 0");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   silo_gpu_distinct_part mine{};
   if (const int status = checkSelection("silo_gpu_distinct_classes", table_dev, slots, parts_dev, n_parts, part, filter_dev, keys_dev, hip_stream, mine);
       status != SILO_GPU_OK) {
      return status;
   }
   const uint32_t step_words = WORDS_PER_BLOCK * CLASS_WORDS;  // of a block
   k_distinct_classes<<<std::min((mine.row_words + step_words - 1u) / step_words, MAX_WALK_BLOCKS), THREADS, 0, hip_stream>>>(
      static_cast<uint32_t*>(table_dev), slots, counts_dev, parts_dev, n_parts, part, filter_dev, min_count, keys_dev, capacity, n_keys_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_smallest_keys(
   const uint64_t* keys_dev, const uint32_t* n_keys_dev, uint32_t capacity, uint32_t k, uint64_t* out_dev, uint32_t* out_count_dev, void* scratch_dev,
   void* stream
) {
   if (keys_dev == nullptr || n_keys_dev == nullptr || out_dev == nullptr || out_count_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_smallest_keys: bad arguments");
   }
   if (capacity == 0 || k == 0 || k > SILO_GPU_MAX_DISTINCT_CLASSES) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_smallest_keys: a capacity of 0, or k outside 1 .. SILO_GPU_MAX_DISTINCT_CLASSES");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   auto* scratch = static_cast<uint32_t*>(scratch_dev);
   const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(capacity) + THREADS - 1u) / THREADS, MAX_KEY_BLOCKS));
   HIP_TRY(hipMemsetAsync(scratch, 0, SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES, hip_stream));  // no histogram, no prefix, nothing appended
   for (uint32_t round = 0; round < KEY_ROUNDS; ++round) {
      k_keys_histogram<<<blocks, THREADS, 0, hip_stream>>>(keys_dev, n_keys_dev, capacity, scratch, round);
      HIP_TRY(hipGetLastError());
      k_keys_advance<<<1, THREADS, 0, hip_stream>>>(n_keys_dev, capacity, k, scratch, round, out_count_dev);
      HIP_TRY(hipGetLastError());
   }
   k_keys_gather<<<blocks, THREADS, 0, hip_stream>>>(keys_dev, n_keys_dev, capacity, k, scratch, out_dev);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
