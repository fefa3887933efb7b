// silo_gpu_neighbours.hip — the k lowest cells of every row of a rectangle of distances behind NearestAmong (K14):
// for the cells silo_gpu_distance_cross (silo_gpu_distance.hip) leaves, per row the k eligible columns that are lowest by
// (distance, column), ascending.  Takes no store.
//
// Kernel:
//   k_nearest_columns   a block per row: the keys of a thread's cells in registers, then min(k, n_columns) rounds of a block-wide
//                       minimum, each of which lists one column and retires its key (silo_gpu_nearest_columns)
#include "block_minimum.h"
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t NEIGHBOUR_THREADS = SILO_GPU_NEIGHBOUR_THREADS;
constexpr uint32_t NEIGHBOUR_WAVES = NEIGHBOUR_THREADS / 64u;
constexpr uint32_t NEIGHBOUR_OWNED = SILO_GPU_MAX_CROSS_COLUMNS / NEIGHBOUR_THREADS;  // columns per thread, at the limit
constexpr uint32_t COLUMN_BITS = SILO_GPU_NEIGHBOUR_KEY_COLUMN_BITS;
constexpr uint64_t NO_KEY = UINT64_MAX;
static_assert(NEIGHBOUR_OWNED * NEIGHBOUR_THREADS == SILO_GPU_MAX_CROSS_COLUMNS && NEIGHBOUR_OWNED <= 8);
static_assert(SILO_GPU_MAX_CROSS_COLUMNS == 1u << COLUMN_BITS);

/// grid = n_rows, block i owns row i.  Thread t owns the columns t, t + THREADS, ...: keys[c] is `distance << 13 | column` of its
/// c-th column — a strict order, (distance, column) — and NO_KEY where the cell is not eligible (its distance is UINT32_MAX) or the
/// column is at or past n_columns; consecutive threads read consecutive cells, all loads of a thread in flight.  Then exactly
/// min(k, n_columns) rounds: the block-wide minimum of every thread's lowest key (blockMinimum, two sets of partials in turn: one
/// barrier per round) is the same in every thread; NO_KEY lists nothing (and so does every round after it); otherwise the one
/// thread that holds the key — keys are distinct — reads `compared` from that cell, stores entry `listed` and retires the key.
/// Thread 0 stores the count.  The column of an entry is k * THREADS + threadIdx.x of its owner: nothing read from the cells is
/// used as an index, and every loop has a trip count fixed by k and n_columns.
__global__ __launch_bounds__(NEIGHBOUR_THREADS) void k_nearest_columns(
   const uint32_t* __restrict__ cells, uint32_t n_columns, uint32_t k, uint32_t* __restrict__ out, uint32_t* __restrict__ counts
) {
   __shared__ uint64_t s_partial[2][NEIGHBOUR_WAVES];
   const uint32_t* row = cells + static_cast<size_t>(blockIdx.x) * n_columns * 2u;
   uint32_t* list = out + static_cast<size_t>(blockIdx.x) * k * 3u;
   uint64_t keys[NEIGHBOUR_OWNED];
#pragma unroll
   for (uint32_t c = 0; c < NEIGHBOUR_OWNED; ++c) {
      const uint32_t column = c * NEIGHBOUR_THREADS + threadIdx.x;
      const uint32_t distance = column < n_columns ? row[static_cast<size_t>(column) * 2u] : UINT32_MAX;
      keys[c] = distance != UINT32_MAX ? (static_cast<uint64_t>(distance) << COLUMN_BITS) | column : NO_KEY;
   }
   const uint32_t rounds = min(k, n_columns);
   uint32_t listed = 0;
   for (uint32_t round = 0; round < rounds; ++round) {
      uint64_t lowest = NO_KEY;
#pragma unroll
      for (uint32_t c = 0; c < NEIGHBOUR_OWNED; ++c) {
         lowest = min(lowest, keys[c]);
      }
      lowest = blockMinimum<NEIGHBOUR_WAVES>(lowest, s_partial[round & 1u]);
      if (lowest != NO_KEY) {  // uniform
#pragma unroll
         for (uint32_t c = 0; c < NEIGHBOUR_OWNED; ++c) {
            if (keys[c] == lowest) {
               const uint32_t column = c * NEIGHBOUR_THREADS + threadIdx.x;  // < n_columns: the key is of a cell that was read
               uint32_t* entry = list + static_cast<size_t>(listed) * 3u;
               entry[0] = column;
               entry[1] = static_cast<uint32_t>(lowest >> COLUMN_BITS);
               entry[2] = row[static_cast<size_t>(column) * 2u + 1u];
               keys[c] = NO_KEY;
            }
         }
         ++listed;
      }
   }
   if (threadIdx.x == 0) {
      counts[blockIdx.x] = listed;
   }
}

}  // namespace

extern "C" {

int silo_gpu_nearest_columns(
   const uint32_t* cells_dev, uint32_t n_rows, uint32_t n_columns, uint32_t k, uint32_t* out_dev, uint32_t* counts_dev, void* stream
) {
   if (cells_dev == nullptr || out_dev == nullptr || counts_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_columns: a buffer is NULL");
   }
   if (k == 0 || k > SILO_GPU_MAX_NEIGHBOUR_COLUMNS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_columns: k is 0 or more than SILO_GPU_MAX_NEIGHBOUR_COLUMNS");
   }
   if (n_rows > SILO_GPU_MAX_CROSS_ROWS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_columns: more rows than SILO_GPU_MAX_CROSS_ROWS");
   }
   if (n_columns > SILO_GPU_MAX_CROSS_COLUMNS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_columns: more columns than SILO_GPU_MAX_CROSS_COLUMNS");
   }
   if (n_rows == 0) {
      return SILO_GPU_OK;
   }
   k_nearest_columns<<<n_rows, NEIGHBOUR_THREADS, 0, static_cast<hipStream_t>(stream)>>>(cells_dev, n_columns, k, out_dev, counts_dev);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
