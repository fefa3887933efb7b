// block_minimum.h — the block-wide minimum of one 64-bit value per thread, as the forest kernel (silo_gpu_spanning.hip) and the
// neighbour kernel (silo_gpu_neighbours.hip) take it once per step.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace silo_gpu_detail {

/// The minimum of `value` over the block of WAVES waves of 64 lanes, the same in every thread: a reduction over the wave, the
/// WAVES partials through `partials` (LDS, WAVES words) and a reduction over those.  ONE barrier: a caller that takes a minimum per
/// step passes two sets of partials in turn, so that a wave that is a step ahead writes the set that nobody reads any more.
template <uint32_t WAVES>
__device__ __forceinline__ uint64_t blockMinimum(uint64_t value, uint64_t* partials) {
   static_assert(WAVES <= 64 && (WAVES & (WAVES - 1u)) == 0);
#pragma unroll
   for (uint32_t offset = 32; offset > 0; offset >>= 1) {
      value = min(value, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(value), static_cast<int>(offset))));
   }
   if ((threadIdx.x & 63u) == 0) {
      partials[threadIdx.x / 64u] = value;
   }
   __syncthreads();
   value = partials[threadIdx.x & (WAVES - 1u)];
#pragma unroll
   for (uint32_t offset = WAVES / 2u; offset > 0; offset >>= 1) {
      value = min(value, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(value), static_cast<int>(offset))));
   }
   return value;
}

}  // namespace silo_gpu_detail
