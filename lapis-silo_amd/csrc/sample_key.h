// sample_key.h — the keyed permutation of row numbers behind Sample (K19), for the host and the kernels alike.
//   key(seed, row) = fmix32(fmix32(row + k1) ^ k2),  k1 / k2 = the low / high 32 bits of splitmix64(seed)
// Every step is a bijection of uint32: two rows never share a key, whatever the seed.
#ifndef SILO_GPU_SAMPLE_KEY_H
#define SILO_GPU_SAMPLE_KEY_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SILO_SAMPLE_KEY_FN __host__ __device__ inline
#else
#define SILO_SAMPLE_KEY_FN inline
#endif

namespace silo_gpu_sample {

/// The finaliser of MurmurHash3.
SILO_SAMPLE_KEY_FN uint32_t fmix32(uint32_t h) {
   h ^= h >> 16;
   h *= 0x85EBCA6Bu;
   h ^= h >> 13;
   h *= 0xC2B2AE35u;
   h ^= h >> 16;
   return h;
}

SILO_SAMPLE_KEY_FN uint64_t splitmix64(uint64_t z) {
   z += 0x9E3779B97F4A7C15ull;
   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
   z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
   return z ^ (z >> 31);
}

/// The key of a row under the round keys of a seed.
SILO_SAMPLE_KEY_FN uint32_t keyOf(uint32_t k1, uint32_t k2, uint32_t global_row) {
   return fmix32(fmix32(global_row + k1) ^ k2);
}

}  // namespace silo_gpu_sample

#endif  // SILO_GPU_SAMPLE_KEY_H
