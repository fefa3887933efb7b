// internal.h — what the translation units of libsilo_gpu.so share (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "silo_gpu.h"

/// Records `message` as this thread's silo_gpu_last_error() and returns `code`.
int silo_gpu_internal_fail(int code, const std::string& message);

/// Sorts n 64-bit keys in device memory ascending, in place (silo_gpu_sort.hip); synchronises the null stream.
int silo_gpu_internal_sort_keys(uint64_t* keys_dev, size_t n);

/// The same by the key bits [begin_bit, end_bit) only; stable (keys equal in those bits keep their order).
int silo_gpu_internal_sort_keys_by_bits(uint64_t* keys_dev, size_t n, int begin_bit, int end_bit);

/// Sorts n (64-bit key, 32-bit value) pairs in device memory by key, ascending, in place; synchronises the null stream.
int silo_gpu_internal_sort_pairs(uint64_t* keys_dev, uint32_t* values_dev, size_t n);

#define SILO_HIP_TRY(expr)                                                                                  \
   do {                                                                                                     \
      hipError_t err_ = (expr);                                                                             \
      if (err_ != hipSuccess) {                                                                             \
         (void)hipGetLastError(); /* clear the sticky error so later launch checks start clean */           \
         return silo_gpu_internal_fail(                                                                     \
            err_ == hipErrorOutOfMemory ? SILO_GPU_ERR_OUT_OF_MEMORY : SILO_GPU_ERR_HIP,                    \
            std::string(#expr) + ": " + hipGetErrorString(err_)                                             \
         );                                                                                                 \
      }                                                                                                     \
   } while (0)

namespace silo_gpu_detail {

/// The owner of one device allocation: alloc() is hipMalloc, and hipFree comes when the owner goes, is reset or is assigned to.
/// Move-only.  Kernels and SeqStoreDev take get().
template <typename T>
class DeviceArray {
  public:
   DeviceArray() = default;
   DeviceArray(DeviceArray&& other) noexcept : ptr_(other.release()) {}
   DeviceArray& operator=(DeviceArray&& other) noexcept {
      if (this != &other) {
         reset();
         ptr_ = other.release();
      }
      return *this;
   }
   DeviceArray(const DeviceArray&) = delete;
   DeviceArray& operator=(const DeviceArray&) = delete;
   ~DeviceArray() { reset(); }
   /// Room for `count` elements; what the owner held before is freed first.
   hipError_t alloc(size_t count) {
      reset();
      const hipError_t status = hipMalloc(&ptr_, count * sizeof(T));
      if (status != hipSuccess) {
         ptr_ = nullptr;
      }
      return status;
   }
   T* get() const { return ptr_; }
   /// Hands the allocation over: the caller frees it.
   T* release() {
      T* ptr = ptr_;
      ptr_ = nullptr;
      return ptr;
   }
   void reset() {
      if (ptr_ != nullptr) {
         (void)hipFree(ptr_);
         ptr_ = nullptr;
      }
   }

  private:
   T* ptr_ = nullptr;
};

/// `bytes` rounded up to the 256-byte alignment of the parts of a scratch buffer.
inline size_t align256(size_t bytes) {
   return (bytes + 255u) / 256u * 256u;
}

/// The blocks of `threads` threads of a grid-stride pass with a thread per item: one thread each up to 4 096 blocks.
inline uint32_t strideBlocks(uint32_t items, uint32_t threads) {
   const uint32_t blocks = (items + threads - 1u) / threads;
   return blocks < 4096u ? blocks : 4096u;
}

/// The blocks of a pass with a wave per row word, `words_per_block` waves to a block.
inline uint32_t blocksOfWords(uint32_t row_words, uint32_t words_per_block) {
   return row_words / words_per_block + (row_words % words_per_block != 0 ? 1u : 0u);
}

}  // namespace silo_gpu_detail
