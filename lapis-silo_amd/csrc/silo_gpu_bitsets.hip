// silo_gpu_bitsets.hip — row bitsets: allocation, upload and download, and the bitsets of a metadata filter made from a
// membership table (lineages of a synthetic store, value ids of a column).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

__global__ __launch_bounds__(256) void k_bitset_from_lineages(
   const uint16_t* __restrict__ lineage, const uint8_t* __restrict__ membership, uint32_t sequence_count,
   uint32_t row_words, uint64_t* __restrict__ out
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t word = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
   if (word >= row_words) {
      return;
   }
   const uint64_t sequence = static_cast<uint64_t>(word) * 64u + lane;
   const bool member = sequence < sequence_count && membership[lineage[sequence]] != 0;
   const uint64_t mask = __ballot(member);
   if (lane == 0) {
      out[word] = mask;
   }
}

__global__ __launch_bounds__(256) void k_bitset_from_value_ids(
   const uint32_t* __restrict__ value_ids, const uint8_t* __restrict__ membership, uint32_t n_values,
   uint32_t sequence_count, uint32_t row_words, uint64_t* __restrict__ out
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t word = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
   if (word >= row_words) {
      return;
   }
   const uint64_t sequence = static_cast<uint64_t>(word) * 64u + lane;
   bool member = false;
   if (sequence < sequence_count) {
      const uint32_t value = value_ids[sequence];
      member = value < n_values && membership[value] != 0;
   }
   const uint64_t mask = __ballot(member);
   if (lane == 0) {
      out[word] = mask;
   }
}

/// Uploads a membership table of `n` bytes, runs `launch` on it (it enqueues `kernel` on the stream) and waits for the stream.
template <typename Launch>
int bitsetFromMembership(const uint8_t* membership, uint32_t n, hipStream_t hip_stream, const char* kernel, Launch launch) {
   DeviceArray<uint8_t> d_membership;
   HIP_TRY(d_membership.alloc(n));
   hipError_t err = hipMemcpyAsync(d_membership.get(), membership, n, hipMemcpyHostToDevice, hip_stream);
   if (err == hipSuccess) {
      launch(d_membership.get());
      err = hipStreamSynchronize(hip_stream);
   }
   if (err != hipSuccess) {
      return fail(SILO_GPU_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(err));
   }
   return SILO_GPU_OK;  // the table is freed here, behind the wait
}

}  // namespace

extern "C" {

int silo_gpu_bitset_alloc(const silo_gpu_store* store, uint64_t** out_dev) {
   if (store == nullptr || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_alloc: bad arguments");
   }
   HIP_TRY(hipSetDevice(store->device));
   const size_t bytes = static_cast<size_t>(store->row_words) * sizeof(uint64_t);
   DeviceArray<uint64_t> bitset;
   HIP_TRY(bitset.alloc(store->row_words));
   HIP_TRY(hipMemset(bitset.get(), 0, bytes));
   HIP_TRY(hipStreamSynchronize(nullptr));  // the fill is enqueued on the null stream; the caller's stream would not wait for it
   *out_dev = bitset.release();
   return SILO_GPU_OK;
}

int silo_gpu_bitset_upload(const silo_gpu_store* store, uint64_t* dst_dev, const uint64_t* src_host, size_t n_words, void* stream) {
   if (store == nullptr || dst_dev == nullptr || src_host == nullptr || n_words > store->row_words) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_upload: bad arguments");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   HIP_TRY(hipMemsetAsync(dst_dev, 0, static_cast<size_t>(store->row_words) * sizeof(uint64_t), hip_stream));
   HIP_TRY(hipMemcpyAsync(dst_dev, src_host, n_words * sizeof(uint64_t), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));
   return SILO_GPU_OK;
}

int silo_gpu_bitset_download(const silo_gpu_store* store, uint64_t* dst_host, const uint64_t* src_dev, size_t n_words, void* stream) {
   if (store == nullptr || dst_host == nullptr || src_dev == nullptr || n_words > store->row_words) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_download: bad arguments");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   HIP_TRY(hipMemcpyAsync(dst_host, src_dev, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));
   return SILO_GPU_OK;
}

int silo_gpu_bitset_from_lineages(const silo_gpu_store* store, uint64_t* dst_dev, const uint8_t* membership_by_lineage, uint32_t n_lineages, void* stream) {
   if (store == nullptr || dst_dev == nullptr || membership_by_lineage == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_from_lineages: bad arguments");
   }
   if (store->d_lineage.get() == nullptr || n_lineages != store->n_lineages) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "store holds no synthetic lineage assignment of that size");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   const uint32_t threads = store->row_words * 64u;
   return bitsetFromMembership(membership_by_lineage, n_lineages, hip_stream, "k_bitset_from_lineages", [&](const uint8_t* d_membership) {
      k_bitset_from_lineages<<<(threads + 255) / 256, 256, 0, hip_stream>>>(
         store->d_lineage.get(), d_membership, store->sequence_count, store->row_words, dst_dev
      );
   });
}

int silo_gpu_bitset_from_value_ids(const silo_gpu_store* store, uint64_t* dst_dev, const uint32_t* value_ids_dev, const uint8_t* membership_by_value, uint32_t n_values, void* stream) {
   if (store == nullptr || dst_dev == nullptr || value_ids_dev == nullptr || membership_by_value == nullptr || n_values == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_from_value_ids: bad arguments");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   const uint32_t threads = store->row_words * 64u;
   return bitsetFromMembership(membership_by_value, n_values, hip_stream, "k_bitset_from_value_ids", [&](const uint8_t* d_membership) {
      k_bitset_from_value_ids<<<(threads + 255) / 256, 256, 0, hip_stream>>>(
         value_ids_dev, d_membership, n_values, store->sequence_count, store->row_words, dst_dev
      );
   });
}

}  // extern "C"
