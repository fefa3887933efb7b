// silo_gpu_planes.hip — the plane of a single symbol at a position, decoded from the store (filter leaves), and FastaAligned
// (k_reconstruct_sequences).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

/// The plane of the missing symbol at one position out of its runs: one thread per run (`out` zeroed beforehand).
__global__ __launch_bounds__(256) void k_runs_to_plane(
   const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ run_ends, uint32_t n_runs, uint32_t position, uint64_t* __restrict__ out
) {
   const uint32_t run = blockIdx.x * blockDim.x + threadIdx.x;
   if (run >= n_runs) {
      return;
   }
   const uint64_t key = run_keys[run];
   if (static_cast<uint32_t>(key) <= position && position < run_ends[run]) {
      const uint32_t sequence = static_cast<uint32_t>(key >> 32);
      atomicOr(reinterpret_cast<unsigned long long*>(out + (sequence >> 6)), 1ull << (sequence & 63u));
   }
}

/// Does `sequence` have the missing symbol at `position`?  The last run that starts at or before the cell decides.
__device__ __forceinline__ bool missingInRuns(const SeqStoreDev& store, uint32_t sequence, uint32_t position) {
   const uint64_t cell = (static_cast<uint64_t>(sequence) << 32) | position;
   uint32_t lo = 0, hi = store.n_missing_runs;
   while (lo < hi) {  // first run whose (sequence, start) is beyond the cell
      const uint32_t mid = lo + (hi - lo) / 2;
      if (store.missing_run_keys[mid] <= cell) {
         lo = mid + 1;
      } else {
         hi = mid;
      }
   }
   if (lo == 0) {
      return false;
   }
   const uint64_t key = store.missing_run_keys[lo - 1];
   return static_cast<uint32_t>(key >> 32) == sequence && position < store.missing_run_ends[lo - 1];
}

// FastaAligned: one thread per (requested row, position) looks the row's bit up in every dense plane of the
// position; a cell no dense plane claims holds a sparsely stored symbol (IUPAC code) and is found by binary search
// for position << 37 | symbol << 32 | sequence in the sorted sparse keys.  A gather (one 8-byte word per plane),
// sized for the <= 10 000 rows the action allows.
__global__ __launch_bounds__(256) void k_reconstruct_sequences(
   const SeqStoreDev store, const uint64_t* __restrict__ sparse_keys, uint32_t n_sparse, const uint32_t* __restrict__ row_ids,
   const char* __restrict__ symbol_chars, char* __restrict__ out
) {
   const uint32_t position = blockIdx.x * blockDim.x + threadIdx.x;
   if (position >= store.positions) {
      return;
   }
   const uint32_t sequence = row_ids[blockIdx.y];
   const uint32_t word = sequence >> 6;
   const uint32_t bit = sequence & 63u;
   uint32_t found = 0xFFu;
   // the row's code in the position's planes, and the valid mutation symbol that code stands for there (0 = none coded)
   const PositionLayout layout = layoutOf(store, position);
   const uint32_t code = codeOfRow(layout, store.row_words, word, bit);
   const uint32_t coded_index = code == 0 ? 0xFFu : (layout.identity ? code - 1u : layout.map[code]);
   for (uint32_t symbol = 0; symbol < store.n_symbols; ++symbol) {
      if (store.kind[symbol] == PLANE_SCAN) {
         if (store.index[symbol] == coded_index) {
            found = symbol;
         }
         continue;
      }
      if (store.kind[symbol] == PLANE_RUNS) {
         if (missingInRuns(store, sequence, position)) {
            found = symbol;
         }
         continue;
      }
      const uint64_t* plane = planePtr(store, position, symbol);
      if (plane != nullptr && ((plane[word] >> bit) & 1u) != 0) {
         found = symbol;
      }
   }
   const auto listed = [&](const uint64_t* keys, uint32_t lo, uint32_t hi, uint64_t key) {  // binary search in keys[lo, hi)
      const uint32_t end = hi;
      while (lo < hi) {
         const uint32_t mid = lo + (hi - lo) / 2;
         if (keys[mid] < key) {
            lo = mid + 1;
         } else {
            hi = mid;
         }
      }
      return lo < end && keys[lo] == key;
   };
   if (found == 0xFFu && store.escapes != nullptr) {  // a valid symbol that has no code at this position: an escape key
      const uint32_t first = store.escape_first[position];
      const uint32_t last = store.escape_first[position + 1];
      for (uint32_t symbol = 0; symbol < store.n_symbols && found == 0xFFu && first < last; ++symbol) {
         if (store.kind[symbol] == PLANE_SCAN &&
             listed(store.escapes, first, last, (static_cast<uint64_t>(position) << 37) | (static_cast<uint64_t>(store.index[symbol]) << 32) | sequence)) {
            found = symbol;
         }
      }
   }
   if (found == 0xFFu) {
      for (uint32_t symbol = 0; symbol < store.n_symbols && found == 0xFFu; ++symbol) {
         if (store.kind[symbol] == PLANE_SPARSE &&
             listed(sparse_keys, 0, n_sparse, (static_cast<uint64_t>(position) << 37) | (static_cast<uint64_t>(symbol) << 32) | sequence)) {
            found = symbol;
         }
      }
   }
   if (found == 0xFFu && layout.implicit) {  // no other symbol claims the cell: the position's derived symbol
      for (uint32_t symbol = 0; symbol < store.n_symbols; ++symbol) {
         if (store.kind[symbol] == PLANE_SCAN && store.index[symbol] == layout.map[IMPLICIT_SLOT]) {
            found = symbol;
         }
      }
   }
   out[static_cast<size_t>(blockIdx.y) * store.positions + position] = found == 0xFFu ? '?' : symbol_chars[found];
}

// One-hot plane of a valid mutation symbol out of the position's code planes (2, 3 or n_bits reads per word); a symbol
// that has no code at the position yields zeros (its rows are escape keys: the caller scatters them on top).
__global__ __launch_bounds__(256) void k_decode_plane(
   const SeqStoreDev store, uint32_t position, uint32_t symbol, const uint64_t* __restrict__ valid_words, uint64_t* __restrict__ out
) {
   const uint32_t word = blockIdx.x * blockDim.x + threadIdx.x;
   if (word < store.row_words) {
      const PositionLayout layout = layoutOf(store, position);
      const uint32_t code = codeOfSymbol(layout, store.index[symbol]);
      if (code == CODE_IMPLICIT) {  // the derived symbol: every row no stored row claims (the caller clears the keys, the runs, the sparse symbols)
         uint64_t others = 0;
         for (uint32_t row = 0; row < layout.bits; ++row) {
            others |= layout.rows[static_cast<size_t>(row) * store.row_words + word];
         }
         out[word] = ~others & valid_words[word];
         return;
      }
      out[word] = code == CODE_ESCAPED ? 0ull : decodeCodeWord(layout, store.row_words, code, word);
   }
}

/// Clears the rows of keys[begin, end) (sequence in the low 32 bits) in `out`.
__global__ void k_clear_keys(const uint64_t* __restrict__ keys, uint32_t begin, uint32_t end, uint64_t* out) {
   const uint32_t k = begin + blockIdx.x * blockDim.x + threadIdx.x;
   if (k < end) {
      const uint32_t sequence = static_cast<uint32_t>(keys[k] & 0xFFFFFFFFull);
      atomicAnd(reinterpret_cast<unsigned long long*>(out + (sequence >> 6)), ~(1ull << (sequence & 63u)));
   }
}

/// Clears the rows whose run of the missing symbol covers `position` in `out`.
__global__ __launch_bounds__(256) void k_runs_clear_plane(
   const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ run_ends, uint32_t n_runs, uint32_t position, uint64_t* __restrict__ out
) {
   const uint32_t run = blockIdx.x * blockDim.x + threadIdx.x;
   if (run >= n_runs) {
      return;
   }
   const uint64_t key = run_keys[run];
   if (static_cast<uint32_t>(key) <= position && position < run_ends[run]) {
      const uint32_t sequence = static_cast<uint32_t>(key >> 32);
      atomicAnd(reinterpret_cast<unsigned long long*>(out + (sequence >> 6)), ~(1ull << (sequence & 63u)));
   }
}

__global__ void k_scatter_sparse(const uint64_t* __restrict__ keys, uint32_t begin, uint32_t end, uint64_t* out) {
   const uint32_t k = begin + blockIdx.x * blockDim.x + threadIdx.x;
   if (k < end) {
      const uint32_t sequence = static_cast<uint32_t>(keys[k] & 0xFFFFFFFFull);
      atomicOr(reinterpret_cast<unsigned long long*>(out + (sequence >> 6)), 1ull << (sequence & 63u));
   }
}

}  // namespace

extern "C" {

const uint64_t* silo_gpu_store_plane(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t position, uint32_t symbol) {
   if (store == nullptr || seqstore_id >= store->seqstores.size()) {
      return nullptr;
   }
   const SeqStoreDev& dev = store->seqstores[seqstore_id].dev;
   if (position >= dev.positions || symbol >= dev.n_symbols) {
      return nullptr;
   }
   return planePtr(dev, position, symbol);
}

int silo_gpu_store_sparse_plane(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t position, uint32_t symbol, uint64_t* dst_dev, void* stream) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || dst_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_sparse_plane: bad arguments");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (position >= seqstore.dev.positions || symbol >= seqstore.dev.n_symbols) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "position or symbol out of range");
   }
   if (!seqstore.finalized) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "store not finalized");
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (seqstore.dev.kind[symbol] == PLANE_SCAN) {  // a valid mutation symbol: decode its one-hot plane from the position's code planes
      k_decode_plane<<<(store->row_words + 255) / 256, 256, 0, hip_stream>>>(seqstore.dev, position, symbol, store->d_ones.get(), dst_dev);
      HIP_TRY(hipGetLastError());
      const uint8_t* map = seqstore.layout.code_map.empty() ? nullptr : seqstore.layout.code_map.data() + static_cast<size_t>(position) * CODE_MAP_STRIDE;
      if (map != nullptr && (map[0] & LAYOUT_IMPLICIT) != 0 && map[IMPLICIT_SLOT] == seqstore.dev.index[symbol]) {
         // the position's derived symbol: "no other symbol and not missing" (the reference rebuilds its deleted bitmap the same way,
         // nucleotide_symbol_equals.cpp:158-180) — the kernel took the stored rows away; now the keys, the runs, the ambiguity codes
         const uint32_t key_begin = seqstore.layout.escape_first[position];
         const uint32_t key_end = seqstore.layout.escape_first[position + 1];
         if (key_end > key_begin) {
            k_clear_keys<<<(key_end - key_begin + 255) / 256, 256, 0, hip_stream>>>(seqstore.layout.d_escapes.get(), key_begin, key_end, dst_dev);
         }
         if (seqstore.dev.n_missing_runs > 0) {
            k_runs_clear_plane<<<(seqstore.dev.n_missing_runs + 255) / 256, 256, 0, hip_stream>>>(
               seqstore.dev.missing_run_keys, seqstore.dev.missing_run_ends, seqstore.dev.n_missing_runs, position, dst_dev
            );
         }
         const auto lo = std::lower_bound(seqstore.sparse_sorted.begin(), seqstore.sparse_sorted.end(), static_cast<uint64_t>(position) << 37);
         const auto hi = std::lower_bound(lo, seqstore.sparse_sorted.end(), (static_cast<uint64_t>(position) + 1) << 37);
         if (hi > lo) {
            const uint32_t begin = static_cast<uint32_t>(lo - seqstore.sparse_sorted.begin());
            const uint32_t end = static_cast<uint32_t>(hi - seqstore.sparse_sorted.begin());
            k_clear_keys<<<(end - begin + 255) / 256, 256, 0, hip_stream>>>(seqstore.d_sparse.get(), begin, end, dst_dev);
         }
         HIP_TRY(hipGetLastError());
         return SILO_GPU_OK;
      }
      if (!seqstore.layout.escape_first_symbol.empty()) {  // rows of the symbol that are listed as escape keys (it has no code here)
         const size_t counter = static_cast<size_t>(position) * seqstore.dev.n_scan + seqstore.dev.index[symbol];
         const uint32_t begin = seqstore.layout.escape_first_symbol[counter];
         const uint32_t end = seqstore.layout.escape_first_symbol[counter + 1];
         if (end > begin) {
            k_scatter_sparse<<<(end - begin + 255) / 256, 256, 0, hip_stream>>>(seqstore.layout.d_escapes.get(), begin, end, dst_dev);
            HIP_TRY(hipGetLastError());
         }
      }
      return SILO_GPU_OK;
   }
   if (seqstore.dev.kind[symbol] == PLANE_RUNS) {  // the missing symbol: its runs that cover the position
      HIP_TRY(hipMemsetAsync(dst_dev, 0, static_cast<size_t>(store->row_words) * sizeof(uint64_t), hip_stream));
      const uint32_t n_runs = seqstore.dev.n_missing_runs;
      if (n_runs > 0) {
         k_runs_to_plane<<<(n_runs + 255) / 256, 256, 0, hip_stream>>>(seqstore.dev.missing_run_keys, seqstore.dev.missing_run_ends, n_runs, position, dst_dev);
         HIP_TRY(hipGetLastError());
      }
      return SILO_GPU_OK;
   }
   if (seqstore.dev.kind[symbol] == PLANE_EXTRA) {  // already a plane: copy it
      HIP_TRY(hipMemcpyAsync(
         dst_dev, planePtr(seqstore.dev, position, symbol), static_cast<size_t>(store->row_words) * sizeof(uint64_t), hipMemcpyDeviceToDevice,
         hip_stream
      ));
      return SILO_GPU_OK;
   }
   HIP_TRY(hipMemsetAsync(dst_dev, 0, static_cast<size_t>(store->row_words) * sizeof(uint64_t), hip_stream));
   const uint64_t key_begin = (static_cast<uint64_t>(position) << 37) | (static_cast<uint64_t>(symbol) << 32);
   const uint64_t key_end = key_begin + (1ull << 32);
   const auto lo = std::lower_bound(seqstore.sparse_sorted.begin(), seqstore.sparse_sorted.end(), key_begin);
   const auto hi = std::lower_bound(lo, seqstore.sparse_sorted.end(), key_end);
   const uint32_t begin = static_cast<uint32_t>(lo - seqstore.sparse_sorted.begin());
   const uint32_t end = static_cast<uint32_t>(hi - seqstore.sparse_sorted.begin());
   if (end > begin) {
      k_scatter_sparse<<<(end - begin + 255) / 256, 256, 0, hip_stream>>>(seqstore.d_sparse.get(), begin, end, dst_dev);
      HIP_TRY(hipGetLastError());
   }
   return SILO_GPU_OK;
}

int silo_gpu_reconstruct_sequences(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint32_t* row_ids_dev, uint32_t n_rows, char* out_chars_dev, void* stream
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || row_ids_dev == nullptr || out_chars_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_reconstruct_sequences: bad arguments");
   }
   if (n_rows > 65535) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_reconstruct_sequences: at most 65535 rows per call");
   }
   HIP_TRY(hipSetDevice(store->device));
   auto* mutable_store = const_cast<silo_gpu_store*>(store);  // the symbol -> char table is created on first use
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (!seqstore.finalized) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_reconstruct_sequences: store is not finalized");
   }
   if (n_rows == 0 || seqstore.dev.positions == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t alphabet = seqstore.alphabet == SILO_GPU_ALPHABET_AMINO_ACID ? 1 : 0;
   {
      const std::lock_guard<std::mutex> lock(mutable_store->mutex);
      if (mutable_store->d_symbol_chars[alphabet].get() == nullptr) {
         // enum order of the reference's alphabets (nucleotide_symbols.h:15-34, aa_symbols.h:15-43)
         const char* chars = alphabet == 0 ? "-ACGTRYSWKMBDHVN" : "-ACDEFGHIKLMNPQRSTVWYBZ*X";
         DeviceArray<char> device;
         HIP_TRY(device.alloc(SILO_GPU_MAX_SYMBOLS));
         HIP_TRY(hipMemcpy(device.get(), chars, strlen(chars), hipMemcpyHostToDevice));
         mutable_store->d_symbol_chars[alphabet] = std::move(device);
      }
   }
   const dim3 grid((seqstore.dev.positions + 255) / 256, n_rows);
   k_reconstruct_sequences<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(
      seqstore.dev, seqstore.d_sparse.get(), static_cast<uint32_t>(seqstore.sparse_sorted.size()), row_ids_dev,
      store->d_symbol_chars[alphabet].get(), out_chars_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
