// silo_gpu_spanning.hip — the minimum spanning forest behind MinimumSpanningTree (K13): for a symmetric matrix of
// weights over n rows, as silo_gpu_distance_weights (silo_gpu_distance.hip) leaves it, the keys of the forest's edges, ascending.
// Takes no store.
//
// Kernel:
//   k_spanning_forest   ONE block: Prim's algorithm with a restart — the best key of every vertex in a register of its thread, per
//                       step one row of the matrix and one block-wide minimum — then a bitonic sort of the keys in LDS
//                       (silo_gpu_spanning_forest)
#include "block_minimum.h"
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t SPANNING_THREADS = SILO_GPU_SPANNING_THREADS;
constexpr uint32_t SPANNING_WAVES = SPANNING_THREADS / 64u;
constexpr uint32_t SPANNING_MAX_ROWS = SILO_GPU_MAX_SPANNING_ROWS;
constexpr uint32_t SPANNING_OWNED = SPANNING_MAX_ROWS / SPANNING_THREADS;  // vertices per thread, at the limit
constexpr uint32_t ROW_BITS = SILO_GPU_SPANNING_KEY_ROW_BITS;
constexpr uint32_t ROW_MASK = SPANNING_MAX_ROWS - 1u;
constexpr uint64_t NO_KEY = UINT64_MAX;
/// What a vertex outside the forest offers to the block-wide minimum: `key << 1 | (the vertex is the key's j)` if it has a key —
/// below 2^59, in the order of the keys — and RESTART | vertex if it has none: above every key, the lowest vertex first.
constexpr uint64_t RESTART = uint64_t{1} << 62;
static_assert(SPANNING_OWNED * SPANNING_THREADS == SPANNING_MAX_ROWS && SPANNING_OWNED <= 8);
static_assert(SPANNING_MAX_ROWS == 1u << ROW_BITS && SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT == 2u * ROW_BITS);
static_assert(SPANNING_WAVES <= 64 && (SPANNING_WAVES & (SPANNING_WAVES - 1u)) == 0);

/// One block.  Thread t owns the vertices t, t + THREADS, ...; best[k] is the lowest key among the edges from its k-th vertex into
/// the forest (NO_KEY: none), in_forest its vertices that are in.  Vertex 0 starts the forest.  A step, n_rows - 1 of them: the
/// block reads row u of the matrix, u the vertex that entered last — consecutive threads, consecutive cells, all loads of a thread
/// in flight — and lowers best[] of its vertices outside the forest with one compare each; the minimum of what these vertices
/// offer (see RESTART) goes through a wave reduction and SPANNING_WAVES partials in LDS (blockMinimum, block_minimum.h), two sets
/// of them in turn so that one barrier per step is enough.  Every thread then holds the same minimum: a key — thread 0 appends it
/// to s_keys, and the key's end outside the forest, which the low bit names, enters — or no key at all, and the lowest vertex outside enters without an edge.
/// Keys are distinct (an unordered pair has one), so the order is strict and Prim's choice is the unique forest's.  Every vertex
/// index comes from threadIdx and the loop counters, never from the matrix, whose cells only become the high bits of a key; every
/// loop has a trip count fixed by n_rows.  Then s_keys, padded with NO_KEY to a power of two, is sorted (bitonic, a barrier per
/// pass) and stored.
__global__ __launch_bounds__(SPANNING_THREADS) void k_spanning_forest(
   const uint32_t* __restrict__ weights, uint32_t n_rows, uint64_t* __restrict__ edges, uint32_t* __restrict__ count_out
) {
   __shared__ uint64_t s_keys[SPANNING_MAX_ROWS];
   __shared__ uint64_t s_partial[2][SPANNING_WAVES];
   uint64_t best[SPANNING_OWNED];
#pragma unroll
   for (uint32_t k = 0; k < SPANNING_OWNED; ++k) {
      best[k] = NO_KEY;
   }
   uint32_t in_forest = threadIdx.x == 0 ? 1u : 0u;
   uint32_t u = 0;
   uint32_t count = 0;
   for (uint32_t step = 1; step < n_rows; ++step) {
      const uint32_t* row = weights + static_cast<size_t>(u) * n_rows;
      uint32_t cell[SPANNING_OWNED];
#pragma unroll
      for (uint32_t k = 0; k < SPANNING_OWNED; ++k) {
         const uint32_t v = k * SPANNING_THREADS + threadIdx.x;
         cell[k] = v < n_rows ? row[v] : UINT32_MAX;
      }
      uint64_t offer = NO_KEY;
#pragma unroll
      for (uint32_t k = 0; k < SPANNING_OWNED; ++k) {
         const uint32_t v = k * SPANNING_THREADS + threadIdx.x;
         if (v < n_rows && ((in_forest >> k) & 1u) == 0) {
            if (cell[k] != UINT32_MAX) {  // (v != u: u is in the forest)
               best[k] = min(best[k], SILO_GPU_SPANNING_KEY(cell[k], min(u, v), max(u, v)));
            }
            const uint64_t mine = best[k] != NO_KEY ? (best[k] << 1) | ((best[k] & ROW_MASK) == v ? 1u : 0u) : RESTART | v;
            offer = min(offer, mine);
         }
      }
      offer = blockMinimum<SPANNING_WAVES>(offer, s_partial[step & 1u]);
      // step < n_rows: a vertex is outside the forest, so `offer` is a key's or a restart's, the same in every thread
      if (offer < RESTART) {
         const uint64_t key = offer >> 1;
         if (threadIdx.x == 0) {
            s_keys[count] = key;
         }
         ++count;
         u = static_cast<uint32_t>((offer & 1u) != 0 ? key : key >> ROW_BITS) & ROW_MASK;
      } else {
         u = static_cast<uint32_t>(offer) & ROW_MASK;
      }
      u = min(u, n_rows - 1u);  // (it is below n_rows already; said once more where it becomes the row that is read)
      if ((u & (SPANNING_THREADS - 1u)) == threadIdx.x) {
         in_forest |= 1u << (u / SPANNING_THREADS);
      }
   }
   // count <= n_rows - 1 < SPANNING_MAX_ROWS
   uint32_t padded = 1;
   for (uint32_t bit = 0; bit < ROW_BITS && padded < count; ++bit) {
      padded <<= 1;
   }
   __syncthreads();
   for (uint32_t i = count + threadIdx.x; i < padded; i += SPANNING_THREADS) {
      s_keys[i] = NO_KEY;
   }
   __syncthreads();
   for (uint32_t size = 2; size <= padded; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
         for (uint32_t i = threadIdx.x; i < padded; i += SPANNING_THREADS) {
            const uint32_t partner = i ^ stride;
            if (partner > i) {
               const uint64_t a = s_keys[i];
               const uint64_t b = s_keys[partner];
               if ((a > b) == ((i & size) == 0)) {
                  s_keys[i] = b;
                  s_keys[partner] = a;
               }
            }
         }
         __syncthreads();
      }
   }
   for (uint32_t i = threadIdx.x; i < count; i += SPANNING_THREADS) {
      edges[i] = s_keys[i];
   }
   if (threadIdx.x == 0) {
      *count_out = count;
   }
}

}  // namespace

extern "C" {

int silo_gpu_spanning_forest(const uint32_t* weights_dev, uint32_t n_rows, uint64_t* edges_dev, uint32_t* count_dev, void* stream) {
   if (weights_dev == nullptr || edges_dev == nullptr || count_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_spanning_forest: a buffer is NULL");
   }
   if (n_rows > SILO_GPU_MAX_SPANNING_ROWS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_spanning_forest: more rows than SILO_GPU_MAX_SPANNING_ROWS");
   }
   if (n_rows == 0) {
      return SILO_GPU_OK;
   }
   k_spanning_forest<<<1, SPANNING_THREADS, 0, static_cast<hipStream_t>(stream)>>>(weights_dev, n_rows, edges_dev, count_dev);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
