// silo_gpu_sample.hip — K19, the filter expression Sample: the `size` rows of a filter with the smallest keys of a seeded
// permutation of row numbers (sample_key.h), per group of rows, over any number of partitions.  A radix select on bitsets: four
// rounds of 8 key bits, most significant first, each a count pass per partition into one histogram [group][256] and one small
// launch that picks every group's digit; then a pass per partition that compares each row's key with its group's threshold.
//   k_sample_groups   a thread per row: the date range of each selected row as uint16 (the conventions of K7's k_assign_groups)
//   k_sample_begin    writes the state: the round keys of the seed, `size` rows to take in every group, histogram 0
//   k_sample_count    a wave per filter word, grid-stride: rows whose key continues their group's prefix add 1 to the cell of
//                     their next digit — in a block's LDS histogram, flushed where not 0 (few groups), or straight into the table
//   k_sample_advance  a block per group: running sums of its 256 cells, the digit where they reach the rows still to take
//   k_sample_select   a thread per row, a wave's ballot per word: key <= the group's threshold, or the whole group
// Nothing returns to the host between the launches; integer atomics only, so the histogram does not depend on the schedule.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "sample_key.h"
#include "store_internal.h"

using namespace silo_gpu_detail;
using silo_gpu_sample::keyOf;

namespace {

constexpr uint32_t NO_GROUP = 0xFFFFu;
constexpr uint32_t THREADS = 256;  // four waves: four filter words per step
constexpr uint32_t WORDS_PER_BLOCK = THREADS / 64u;
constexpr uint32_t DIGITS = 256;  // 8 key bits per round
constexpr uint32_t HEADER_WORDS = 4;  // n_groups, size, k1, k2
constexpr uint32_t GROUP_WORDS = 4;   // prefix, rows still to take, take-all, unused
constexpr uint32_t MAX_COUNT_BLOCKS = 1024;  // of k_sample_count: four per compute unit; each flushes its LDS histogram once
static_assert(THREADS == DIGITS);  // k_sample_advance: a thread per cell of a group
static_assert(SILO_GPU_SAMPLE_STATE_BYTES(3) == (HEADER_WORDS + 3u * (GROUP_WORDS + DIGITS)) * sizeof(uint32_t));
static_assert(SILO_GPU_SAMPLE_ROUNDS * 8 == 32);

enum GroupWord : uint32_t { PREFIX = 0, REMAINING = 1, TAKE_ALL = 2 };

/// Row `lane` of filter word `word` when it counts: selected, a real row, with a group below n_groups.  Otherwise NO_GROUP.
__device__ __forceinline__ uint32_t groupOfRow(
   uint64_t bits, uint64_t row, uint32_t lane, const uint16_t* __restrict__ groups, uint32_t sequence_count, uint32_t n_groups
) {
   if (((bits >> lane) & 1ull) == 0 || row >= sequence_count) {
      return NO_GROUP;
   }
   const uint32_t group = groups != nullptr ? groups[row] : 0u;
   return group < n_groups ? group : NO_GROUP;
}

/// grid = the rows of row_words words in blocks of THREADS.  The ranges, sorted by their start, sit in LDS; a row's group is the
/// range whose start is the last one <= its date, if the date is also <= that range's end.  NULL dates (0) fall in no range.
__global__ __launch_bounds__(THREADS) void k_sample_groups(
   const uint64_t* __restrict__ filter, const uint32_t* __restrict__ dates, const uint32_t* __restrict__ bounds /* from, to, group: [n] each */,
   uint32_t n, uint32_t sequence_count, uint32_t row_words, uint16_t* __restrict__ out
) {
   __shared__ uint32_t s_from[SILO_GPU_MAX_SAMPLE_GROUPS];
   __shared__ uint32_t s_to[SILO_GPU_MAX_SAMPLE_GROUPS];
   __shared__ uint32_t s_group[SILO_GPU_MAX_SAMPLE_GROUPS];
   for (uint32_t i = threadIdx.x; i < n; i += THREADS) {
      s_from[i] = bounds[i];
      s_to[i] = bounds[n + i];
      s_group[i] = bounds[2u * n + i];
   }
   __syncthreads();
   const uint64_t row = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
   if (row >= static_cast<uint64_t>(row_words) * 64u) {
      return;
   }
   uint32_t group = NO_GROUP;
   if (row < sequence_count && ((filter[row >> 6] >> (row & 63u)) & 1ull) != 0) {
      const uint32_t date = dates[row];
      uint32_t lo = 0, hi = n;
      while (lo < hi) {
         const uint32_t mid = (lo + hi) >> 1;
         if (s_from[mid] <= date) {
            lo = mid + 1;
         } else {
            hi = mid;
         }
      }
      if (lo > 0 && date != 0 && date <= s_to[lo - 1]) {  // (every start is >= 1)
         group = s_group[lo - 1];
      }
   }
   out[row] = static_cast<uint16_t>(group);
}

__global__ __launch_bounds__(THREADS) void k_sample_begin(uint32_t* __restrict__ state, uint32_t n_groups, uint32_t size, uint32_t k1, uint32_t k2) {
   const uint32_t words = HEADER_WORDS + n_groups * (GROUP_WORDS + DIGITS);
   const uint32_t word = blockIdx.x * THREADS + threadIdx.x;
   if (word >= words) {
      return;
   }
   uint32_t value = 0;
   if (word < HEADER_WORDS) {
      value = word == 0 ? n_groups : word == 1 ? size : word == 2 ? k1 : k2;
   } else if (word < HEADER_WORDS + n_groups * GROUP_WORDS && (word - HEADER_WORDS) % GROUP_WORDS == REMAINING) {
      value = size;
   }
   state[word] = value;
}

/// grid <= MAX_COUNT_BLOCKS; a wave takes the filter words wave, wave + waves of the grid, ...: one 8-byte load that the whole wave
/// shares, 2 bytes of group per selected row, nothing for a word without a set bit.
__global__ __launch_bounds__(THREADS) void k_sample_count(
   uint32_t* __restrict__ state, const uint64_t* __restrict__ filter, const uint16_t* __restrict__ groups, uint32_t sequence_count,
   uint32_t row_words, uint32_t first_row, uint32_t round
) {
   __shared__ uint32_t s_hist[SILO_GPU_SAMPLE_LDS_GROUPS * DIGITS];
   const uint32_t n_groups = state[0];
   const uint32_t k1 = state[2], k2 = state[3];
   const uint32_t* group_state = state + HEADER_WORDS;
   uint32_t* hist = state + HEADER_WORDS + n_groups * GROUP_WORDS;
   const bool in_lds = n_groups <= SILO_GPU_SAMPLE_LDS_GROUPS;  // (uniform over the launch)
   const uint32_t cells = n_groups * DIGITS;
   if (in_lds) {
      for (uint32_t i = threadIdx.x; i < cells; i += THREADS) {
         s_hist[i] = 0;
      }
      __syncthreads();
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t shift = 24u - 8u * round;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK;
   for (uint64_t word = static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6); word < row_words; word += step) {
      const uint64_t bits = filter[word];
      if (bits == 0) {
         continue;
      }
      const uint64_t row = word * 64u + lane;
      const uint32_t group = groupOfRow(bits, row, lane, groups, sequence_count, n_groups);
      if (group == NO_GROUP) {
         continue;
      }
      const uint32_t key = keyOf(k1, k2, first_row + static_cast<uint32_t>(row));
      if (round != 0) {
         const uint32_t* mine = group_state + group * GROUP_WORDS;
         if (mine[TAKE_ALL] != 0 || (key >> (shift + 8u)) != mine[PREFIX]) {
            continue;
         }
      }
      const uint32_t cell = group * DIGITS + ((key >> shift) & 0xFFu);
      atomicAdd(in_lds ? &s_hist[cell] : &hist[cell], 1u);
   }
   if (in_lds) {
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < cells; i += THREADS) {
         const uint32_t count = s_hist[i];
         if (count != 0) {
            atomicAdd(&hist[i], count);
         }
      }
   }
}

/// grid = SILO_GPU_MAX_SAMPLE_GROUPS blocks (the number of groups is in the state): block g owns group g, thread d its cell d.
__global__ __launch_bounds__(THREADS) void k_sample_advance(uint32_t* __restrict__ state, uint32_t round) {
   __shared__ uint32_t s_sum[DIGITS];
   const uint32_t n_groups = state[0];
   const uint32_t group = blockIdx.x;
   if (group >= n_groups) {
      return;
   }
   const uint32_t size = state[1];
   uint32_t* mine = state + HEADER_WORDS + group * GROUP_WORDS;
   uint32_t* cell = state + HEADER_WORDS + n_groups * GROUP_WORDS + group * DIGITS + threadIdx.x;
   const uint32_t prefix = mine[PREFIX], remaining = mine[REMAINING], take_all = mine[TAKE_ALL];
   const uint32_t count = *cell;
   *cell = 0;
   if (take_all != 0) {  // (uniform over the block; its cells were 0 already)
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
   const uint32_t total = s_sum[DIGITS - 1];
   if (round == 0 && total <= size) {
      if (threadIdx.x == 0) {
         mine[TAKE_ALL] = 1;
      }
      return;
   }
   const uint32_t upto = s_sum[threadIdx.x];
   const uint32_t before = upto - count;
   if (before < remaining && upto >= remaining) {  // one thread (none for size == 0: silo_gpu_sample_select selects nothing then)
      mine[PREFIX] = (prefix << 8) | threadIdx.x;
      mine[REMAINING] = remaining - before;
   }
}

/// A thread per row, a wave per word of the output: a wave whose word is at or past row_words neither loads nor stores.
__global__ __launch_bounds__(THREADS) void k_sample_select(
   const uint32_t* __restrict__ state, const uint64_t* __restrict__ filter, const uint16_t* __restrict__ groups, uint32_t sequence_count,
   uint32_t row_words, uint32_t first_row, uint64_t* __restrict__ out
) {
   const uint64_t row = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
   const uint64_t word = row >> 6;  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t n_groups = state[0];
   const uint32_t size = state[1];
   const uint64_t bits = filter[word];
   bool selected = false;
   if (bits != 0 && size != 0) {
      const uint32_t group = groupOfRow(bits, row, lane, groups, sequence_count, n_groups);
      if (group != NO_GROUP) {
         const uint32_t* mine = state + HEADER_WORDS + group * GROUP_WORDS;
         selected = mine[TAKE_ALL] != 0 || keyOf(state[2], state[3], first_row + static_cast<uint32_t>(row)) <= mine[PREFIX];
      }
   }
   const uint64_t ballot = __ballot(selected);
   if (lane == 0) {
      out[word] = ballot;
   }
}

/// What every entry that walks a partition's rows refuses: `what` names the entry.
int checkRows(const char* what, const void* state, const void* filter, const void* out, uint32_t sequence_count, uint32_t row_words, uint32_t first_row) {
   if (state == nullptr || filter == nullptr || out == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": bad arguments");
   }
   if (row_words == 0 || sequence_count > static_cast<uint64_t>(row_words) * 64u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": no row words, or fewer rows than sequence_count");
   }
   if (static_cast<uint64_t>(first_row) + sequence_count > (uint64_t{1} << 32)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(what) + ": first_row + sequence_count exceeds 2^32 rows");
   }
   return SILO_GPU_OK;
}

}  // namespace

extern "C" {

uint32_t silo_gpu_sample_key(uint64_t seed, uint32_t global_row) {
   const uint64_t k = silo_gpu_sample::splitmix64(seed);
   return keyOf(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32), global_row);
}

int silo_gpu_sample_groups(
   const uint64_t* filter_dev, const uint32_t* date_column_dev, const uint32_t* range_bounds, uint32_t n_ranges, uint32_t sequence_count,
   uint32_t row_words, uint16_t* groups_out_dev, void* stream
) {
   if (const int status = checkRows("silo_gpu_sample_groups", date_column_dev, filter_dev, groups_out_dev, sequence_count, row_words, 0); status != SILO_GPU_OK) {
      return status;
   }
   if (range_bounds == nullptr || n_ranges == 0 || n_ranges > SILO_GPU_MAX_SAMPLE_GROUPS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sample_groups: no date ranges, or more than SILO_GPU_MAX_SAMPLE_GROUPS");
   }
   // the ranges by their start; (from, to, group) as three arrays
   std::vector<uint32_t> order(n_ranges);
   std::iota(order.begin(), order.end(), 0u);
   std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return range_bounds[2u * a] < range_bounds[2u * b]; });
   std::vector<uint32_t> table(3u * static_cast<size_t>(n_ranges));
   for (uint32_t k = 0; k < n_ranges; ++k) {
      const uint32_t from = range_bounds[2u * order[k]], to = range_bounds[2u * order[k] + 1u];
      if (from > to) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sample_groups: a date range ends before it starts");
      }
      if (k > 0 && from <= range_bounds[2u * order[k - 1] + 1u]) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sample_groups: date ranges overlap");
      }
      table[k] = std::max<uint32_t>(from, 1u);
      table[n_ranges + k] = to;
      table[2u * n_ranges + k] = order[k];
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   DeviceArray<uint32_t> d_table;
   HIP_TRY(d_table.alloc(table.size()));
   const uint64_t rows = static_cast<uint64_t>(row_words) * 64u;
   hipError_t err = hipMemcpyAsync(d_table.get(), table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, hip_stream);
   if (err == hipSuccess) {
      k_sample_groups<<<static_cast<uint32_t>((rows + THREADS - 1) / THREADS), THREADS, 0, hip_stream>>>(
         filter_dev, date_column_dev, d_table.get(), n_ranges, sequence_count, row_words, groups_out_dev
      );
      err = hipGetLastError();
      const hipError_t waited = hipStreamSynchronize(hip_stream);  // the table is pageable host memory, and its device copy is freed here
      err = err != hipSuccess ? err : waited;
   }
   if (err != hipSuccess) {
      return fail(SILO_GPU_ERR_HIP, std::string("k_sample_groups: ") + hipGetErrorString(err));
   }
   return SILO_GPU_OK;
}

int silo_gpu_sample_begin(void* state_dev, uint32_t n_groups, uint32_t size, uint64_t seed, void* stream) {
   if (state_dev == nullptr || n_groups == 0 || n_groups > SILO_GPU_MAX_SAMPLE_GROUPS || size > static_cast<uint32_t>(INT32_MAX)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sample_begin: no state, a number of groups outside 1 .. SILO_GPU_MAX_SAMPLE_GROUPS, or a size above INT32_MAX");
   }
   const uint64_t k = silo_gpu_sample::splitmix64(seed);
   const uint32_t words = HEADER_WORDS + n_groups * (GROUP_WORDS + DIGITS);
   k_sample_begin<<<(words + THREADS - 1) / THREADS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<uint32_t*>(state_dev), n_groups, size, static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32)
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_sample_count(
   void* state_dev, const uint64_t* filter_dev, const uint16_t* groups_dev, uint32_t sequence_count, uint32_t row_words, uint32_t first_row,
   uint32_t round, void* stream
) {
   if (const int status = checkRows("silo_gpu_sample_count", state_dev, filter_dev, state_dev, sequence_count, row_words, first_row); status != SILO_GPU_OK) {
      return status;
   }
   if (round >= SILO_GPU_SAMPLE_ROUNDS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sample_count: there are rounds 0 .. 3");
   }
   k_sample_count<<<std::min(blocksOfWords(row_words, WORDS_PER_BLOCK), MAX_COUNT_BLOCKS), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<uint32_t*>(state_dev), filter_dev, groups_dev, sequence_count, row_words, first_row, round
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_sample_advance(void* state_dev, uint32_t round, void* stream) {
   if (state_dev == nullptr || round >= SILO_GPU_SAMPLE_ROUNDS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sample_advance: no state, or a round other than 0 .. 3");
   }
   k_sample_advance<<<SILO_GPU_MAX_SAMPLE_GROUPS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(static_cast<uint32_t*>(state_dev), round);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_sample_select(
   const void* state_dev, const uint64_t* filter_dev, const uint16_t* groups_dev, uint32_t sequence_count, uint32_t row_words,
   uint32_t first_row, uint64_t* out_bitset_dev, void* stream
) {
   if (const int status = checkRows("silo_gpu_sample_select", state_dev, filter_dev, out_bitset_dev, sequence_count, row_words, first_row); status != SILO_GPU_OK) {
      return status;
   }
   k_sample_select<<<blocksOfWords(row_words, WORDS_PER_BLOCK), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint32_t*>(state_dev), filter_dev, groups_dev, sequence_count, row_words, first_row, out_bitset_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
