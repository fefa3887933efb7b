// silo_gpu_clusters.hip — the connected components behind Clusters (K12): for a symmetric bit matrix over n rows, as
// silo_gpu_distance_within (silo_gpu_distance.hip) leaves it, per row the lowest row of its component.  Takes no store.
//
// Kernel:
//   k_adjacency_components   ONE block with the labels in LDS: rounds of "a wave per row lowers the row's label, and the label of
//                            its old label, to the lowest label among the row's neighbours", each followed by pointer jumps,
//                            until a round lowers nothing (silo_gpu_adjacency_components)
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t COMPONENTS_THREADS = SILO_GPU_COMPONENTS_THREADS;
constexpr uint32_t COMPONENTS_WAVES = COMPONENTS_THREADS / 64u;
constexpr uint32_t COMPONENTS_MAX_ROWS = SILO_GPU_MAX_CLUSTER_ROWS;
constexpr uint32_t COMPONENTS_WORDS_PER_LANE = SILO_GPU_ADJACENCY_WORDS(COMPONENTS_MAX_ROWS) / 64u;  // of a row, at the limit
constexpr uint32_t COMPONENTS_ROWS_IN_FLIGHT = 4;  // rows whose words a wave loads before it looks at any
static_assert(COMPONENTS_WORDS_PER_LANE * 64u == SILO_GPU_ADJACENCY_WORDS(COMPONENTS_MAX_ROWS));
static_assert(COMPONENTS_MAX_ROWS * sizeof(uint32_t) <= 64u * 1024u);

/// One block.  s_label[i] starts as i.  A round: wave v takes the rows v, v + WAVES, ... in steps of COMPONENTS_ROWS_IN_FLIGHT rows
/// whose words are all loaded first (lane l holds the words l and l + 64 of a row: 512 consecutive bytes per load); a lane walks
/// the set bits of its words — in a row's last word only the bits below n_rows, so a stray bit never indexes s_label — for the
/// lowest label among them, the wave reduces, and lane 0 lowers s_label[row] and s_label[the label the row had] with atomicMin.
/// Then every label is replaced by its label's label until none changes.  The loop ends after a round that lowered nothing, or
/// after n_rows rounds: plain propagation alone needs at most n_rows - 1, so the bound never cuts a run short; it is there so that
/// the loop cannot spin whatever the input holds.
/// Why the fixpoint is the answer whatever the order of the atomics: a label only falls, and s_label[i] is always a row of i's
/// component that is <= i; after a round without a change s_label[i] <= s_label[j] for every set bit (i, j), and the matrix being
/// symmetric, the labels are equal along every edge, so constant on a component — and the lowest row m of a component has
/// s_label[m] <= m in its component, which is m.
__global__ __launch_bounds__(COMPONENTS_THREADS) void k_adjacency_components(
   const uint64_t* __restrict__ adjacency, uint32_t n_rows, uint32_t adjacency_words, uint32_t* __restrict__ labels, uint32_t* __restrict__ rounds_out
) {
   __shared__ uint32_t s_label[COMPONENTS_MAX_ROWS];
   for (uint32_t i = threadIdx.x; i < n_rows; i += COMPONENTS_THREADS) {
      s_label[i] = i;
   }
   __syncthreads();
   const uint32_t wave = threadIdx.x / 64u;
   const uint32_t lane = threadIdx.x & 63u;
   uint32_t rounds = 0;
   while (rounds < n_rows) {
      ++rounds;
      int changed = 0;
      for (uint32_t first = wave; first < n_rows; first += COMPONENTS_WAVES * COMPONENTS_ROWS_IN_FLIGHT) {
         uint64_t bits[COMPONENTS_ROWS_IN_FLIGHT][COMPONENTS_WORDS_PER_LANE];
#pragma unroll
         for (uint32_t r = 0; r < COMPONENTS_ROWS_IN_FLIGHT; ++r) {
            const uint32_t row = first + r * COMPONENTS_WAVES;
#pragma unroll
            for (uint32_t k = 0; k < COMPONENTS_WORDS_PER_LANE; ++k) {
               const uint32_t word = k * 64u + lane;
               bits[r][k] = 0;
               if (row < n_rows && word < adjacency_words) {
                  bits[r][k] = adjacency[static_cast<size_t>(row) * adjacency_words + word];
                  if (word == adjacency_words - 1u && (n_rows & 63u) != 0) {
                     bits[r][k] &= (uint64_t{1} << (n_rows & 63u)) - 1u;
                  }
               }
            }
         }
#pragma unroll
         for (uint32_t r = 0; r < COMPONENTS_ROWS_IN_FLIGHT; ++r) {
            const uint32_t row = first + r * COMPONENTS_WAVES;  // the same for the whole wave
            if (row >= n_rows) {
               break;
            }
            uint32_t lowest = UINT32_MAX;
#pragma unroll
            for (uint32_t k = 0; k < COMPONENTS_WORDS_PER_LANE; ++k) {
               uint64_t rest = bits[r][k];
               while (rest != 0) {
                  const uint32_t neighbour = (k * 64u + lane) * 64u + static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(rest)) - 1);
                  lowest = min(lowest, s_label[neighbour]);
                  rest &= rest - 1u;
               }
            }
#pragma unroll
            for (uint32_t offset = 32; offset > 0; offset >>= 1) {
               lowest = min(lowest, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lowest), static_cast<int>(offset))));
            }
            if (lane == 0) {
               const uint32_t old = s_label[row];
               if (lowest < old) {
                  atomicMin(&s_label[row], lowest);
                  atomicMin(&s_label[old], lowest);
                  changed = 1;
               }
            }
         }
      }
      __syncthreads();
      int jumped;
      do {
         jumped = 0;
         for (uint32_t i = threadIdx.x; i < n_rows; i += COMPONENTS_THREADS) {
            const uint32_t label = s_label[i];
            const uint32_t above = s_label[label];
            if (above < label) {
               atomicMin(&s_label[i], above);
               jumped = 1;
            }
         }
      } while (__syncthreads_or(jumped) != 0);
      if (__syncthreads_or(changed) == 0) {
         break;
      }
   }
   for (uint32_t i = threadIdx.x; i < n_rows; i += COMPONENTS_THREADS) {
      labels[i] = s_label[i];
   }
   if (threadIdx.x == 0 && rounds_out != nullptr) {
      *rounds_out = rounds;
   }
}

}  // namespace

extern "C" {

int silo_gpu_adjacency_components(const uint64_t* adjacency_dev, uint32_t n_rows, uint32_t* labels_dev, uint32_t* rounds_dev, void* stream) {
   if (adjacency_dev == nullptr || labels_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_adjacency_components: a buffer is NULL");
   }
   if (n_rows > SILO_GPU_MAX_CLUSTER_ROWS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_adjacency_components: more rows than SILO_GPU_MAX_CLUSTER_ROWS");
   }
   if (n_rows == 0) {
      return SILO_GPU_OK;
   }
   k_adjacency_components<<<1, COMPONENTS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      adjacency_dev, n_rows, SILO_GPU_ADJACENCY_WORDS(n_rows), labels_dev, rounds_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
