// row_hash.h — the hash term of one cell of an aligned sequence (K20, DistinctSequences), for the host and the kernels alike.
//   x = position * 32 + symbol,  H0 = splitmix64(x),  H1 = splitmix64(x + 2^40)
// A row's hash is the sum of its cells' terms over all positions, mod 2^64 in each of the two lanes: any order of adds gives it.
#ifndef SILO_GPU_ROW_HASH_H
#define SILO_GPU_ROW_HASH_H
#include <stdint.h>

#include "sample_key.h"

namespace silo_gpu_row_hash {

constexpr uint32_t NO_SYMBOL = 31;  // a cell that nothing stored claims (the '?' of k_reconstruct_sequences)
constexpr uint64_t LANE_OFFSET = uint64_t{1} << 40;

/// The term of (position, symbol) in lane 0 or 1.
SILO_SAMPLE_KEY_FN uint64_t term(uint32_t position, uint32_t symbol, uint32_t lane) {
   const uint64_t x = static_cast<uint64_t>(position) * 32u + symbol;
   return silo_gpu_sample::splitmix64(lane == 0 ? x : x + LANE_OFFSET);
}

}  // namespace silo_gpu_row_hash

#endif  // SILO_GPU_ROW_HASH_H
