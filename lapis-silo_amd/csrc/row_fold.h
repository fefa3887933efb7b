// row_fold.h — the pass over a finalized store's adaptive layout that gives every row one 16-byte value, written once for the row
// hashes of K20 (silo_gpu_distinct.hip) and the cell counts of K22 (silo_gpu_cell_counts.hip).  It is the decomposition of K11
// (silo_gpu_nearest.hip): every row gets what the planes say, and each stored thing beside the planes corrects its cell with the
// difference between its symbol and the one the plane pass assumed:
//   foldPlanes    a wave per row word, a lane per row, all positions: the lane's code at the position (code planes, one-hot rows,
//                 extra planes) selects the symbol, an open cell counts as the position's derived symbol or as 31; the row's value
//                 stays in registers and leaves with one 16-byte store per row (zeros for padding rows)
//   foldEscapes   a thread per escape key
//   foldRuns      a thread per run [a, e) of the missing symbol: two lookups in a prefix array of those differences
//   foldSparse    a thread per sparse key (ambiguity code)
// Which symbol a cell holds — the claim rule — is decided here and nowhere else: cellSymbol is what the planes say of one cell, and
// the region values of K23 (silo_gpu_region_counts.hip), which walk position ranges instead of whole rows, call it too, with
// fillBaseSymbols and layoutArgsOf for the tables and arguments it reads.  What a symbol is worth comes from a policy `Fold`, a
// trivially copyable struct passed by value beside the shared arguments:
//   Value                                           the running value of a row, the entry of the prefix array and the 16 bytes stored
//   run_prefix                                      const Value*, [P + 1]: set by foldRows
//   zero()                                          the value of a row without cells
//   add(value, position, symbol)                    one cell more                                                          (device)
//   store(row, value)                               the one 16-byte store of a row                                         (device)
//   correct(row, position, symbol, base)            turns the row's cell at `position` from `base` into `symbol`: atomics   (device)
//   correctRun(row, start, end)                     the same for the missing symbol over [start, end), from run_prefix     (device)
//   nextPrefix(previous, position, base, seqstore)  run_prefix[position + 1] from run_prefix[position]                       (host)
// The instantiations are thin __global__ wrappers with names of their own in the two files (FoldKernels), so that a kernel trace
// tells them apart.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "store_internal.h"

namespace silo_gpu_row_fold {

using namespace silo_gpu_detail;

constexpr uint32_t FOLD_THREADS = 256;  // four waves: four neighbouring row words per block
constexpr uint32_t FOLD_WORDS_PER_BLOCK = FOLD_THREADS / 64u;
constexpr uint32_t MAX_EXTRA = 16;
constexpr uint32_t SCAN_SLOTS = 32;  // scan symbol indices a key can name (5 bits)
constexpr uint8_t NO_SCAN_SYMBOL = 0xFF;
constexpr uint32_t NO_SYMBOL = SILO_GPU_ROW_HASH_NO_SYMBOL;  // a cell that nothing stored claims
static_assert(NO_SYMBOL >= SILO_GPU_MAX_SYMBOLS && NO_SYMBOL < 32u);

/// What the pass needs of a store, whatever it accumulates.
struct LayoutArgs {
   SeqStoreDev dev;
   const uint8_t* base_symbol;   // [P] what the plane pass takes an open cell for: the derived symbol, or NO_SYMBOL
   const uint64_t* sparse_keys;
   uint32_t n_sparse;
   uint32_t n_escapes;
   uint32_t sequence_count;
   uint32_t n_extra;
   uint8_t extra_symbols[MAX_EXTRA];  // symbols kept in extra planes
};

/// The symbol of every scan symbol index, in LDS (a lane looks its own code up): filled by the first SCAN_SLOTS threads.
__device__ __forceinline__ void fillSymbolOfScan(uint8_t* s_symbol_of_scan, const SeqStoreDev& dev) {
   if (threadIdx.x < SCAN_SLOTS) {
      uint32_t found = NO_SCAN_SYMBOL;
      for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {  // (uniform index: scalar loads)
         if (dev.kind[symbol] == PLANE_SCAN && dev.index[symbol] == threadIdx.x) {
            found = symbol;
         }
      }
      s_symbol_of_scan[threadIdx.x] = static_cast<uint8_t>(found);
   }
   __syncthreads();
}

/// What the planes say the cell of row `word * 64 + lane` at `position` holds — the claim rule of the plane pass: the lane's code
/// at the position (code planes, one-hot rows) selects the symbol, an open cell is the position's base symbol, and an extra plane
/// that has the row's bit overrides both.  The plane words of a position are the same for the whole wave: where all of them are
/// 0 — nearly always at a position that derives its symbol — every lane holds the base symbol and the per-lane decode is skipped.
/// `s_symbol_of_scan` is fillSymbolOfScan's table; `has_extra` is args.n_extra != 0 && args.dev.extra != nullptr.
__device__ __forceinline__ uint32_t cellSymbol(
   const LayoutArgs& args, const uint8_t* s_symbol_of_scan, uint32_t position, uint32_t word, uint32_t lane, bool has_extra
) {
   const uint32_t row_words = args.dev.row_words;
   const PositionLayout layout = layoutOf(args.dev, position);
   uint32_t code = 0;
   uint64_t any = 0;
   for (uint32_t plane = 0; plane < layout.bits; ++plane) {
      const uint64_t plane_word = layout.rows[static_cast<size_t>(plane) * row_words + word];
      any |= plane_word;
      const uint32_t set = static_cast<uint32_t>((plane_word >> lane) & 1ull);
      code = layout.one_hot ? (set != 0 ? plane + 1u : code) : (code | (set << plane));
   }
   uint32_t symbol = args.base_symbol[position];
   if (any != 0 && code != 0) {
      const uint32_t scan_index = layout.identity ? code - 1u : (code < CODE_MAP_STRIDE ? layout.map[code] : NO_SCAN_SYMBOL);
      if (scan_index < args.dev.n_scan && scan_index < SCAN_SLOTS) {
         const uint32_t coded = s_symbol_of_scan[scan_index];
         symbol = coded != NO_SCAN_SYMBOL ? coded : symbol;
      }
   }
   if (has_extra) {
      for (uint32_t e = 0; e < args.n_extra; ++e) {
         const uint32_t extra_symbol = args.extra_symbols[e];
         if (((planePtr(args.dev, position, extra_symbol)[word] >> lane) & 1ull) != 0) {
            symbol = extra_symbol;
         }
      }
   }
   return symbol;
}

/// grid = row_words / FOLD_WORDS_PER_BLOCK rounded up: a wave per row word, a lane per row, all positions.
template <typename Fold>
__device__ __forceinline__ void foldPlanes(const LayoutArgs& args, const Fold& fold) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   const uint32_t row_words = args.dev.row_words;
   const uint32_t word = __builtin_amdgcn_readfirstlane(blockIdx.x * FOLD_WORDS_PER_BLOCK + (threadIdx.x >> 6));  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const bool has_extra = args.n_extra != 0 && args.dev.extra != nullptr;
   typename Fold::Value value = Fold::zero();
   for (uint32_t position = 0; position < args.dev.positions; ++position) {
      fold.add(value, position, cellSymbol(args, s_symbol_of_scan, position, word, lane, has_extra));
   }
   const uint64_t row = static_cast<uint64_t>(word) * 64u + lane;
   fold.store(row, row < args.sequence_count ? value : Fold::zero());
}

/// A thread per escape key (grid-stride): a row's valid symbol that has neither a code nor a row at its position.
template <typename Fold>
__device__ __forceinline__ void foldEscapes(const LayoutArgs& args, const Fold& fold) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   for (uint32_t i = blockIdx.x * FOLD_THREADS + threadIdx.x; i < args.n_escapes; i += gridDim.x * FOLD_THREADS) {
      const uint64_t key = args.dev.escapes[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t symbol = s_symbol_of_scan[static_cast<uint32_t>(key >> 32) & 31u];
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count && symbol != NO_SCAN_SYMBOL) {
         fold.correct(row, position, symbol, args.base_symbol[position]);
      }
   }
}

/// A thread per run of the missing symbol (grid-stride).
template <typename Fold>
__device__ __forceinline__ void foldRuns(const LayoutArgs& args, const Fold& fold) {
   for (uint32_t i = blockIdx.x * FOLD_THREADS + threadIdx.x; i < args.dev.n_missing_runs; i += gridDim.x * FOLD_THREADS) {
      const uint64_t key = args.dev.missing_run_keys[i];
      const uint32_t row = static_cast<uint32_t>(key >> 32);
      const uint32_t start = static_cast<uint32_t>(key);
      const uint32_t end = min(args.dev.missing_run_ends[i], args.dev.positions);
      if (start < end && row < args.sequence_count) {
         fold.correctRun(row, start, end);
      }
   }
}

/// A thread per sparse key (grid-stride): an ambiguity code, or the missing symbol where it has neither runs nor a plane.
template <typename Fold>
__device__ __forceinline__ void foldSparse(const LayoutArgs& args, const Fold& fold) {
   for (uint32_t i = blockIdx.x * FOLD_THREADS + threadIdx.x; i < args.n_sparse; i += gridDim.x * FOLD_THREADS) {
      const uint64_t key = args.sparse_keys[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count) {
         fold.correct(row, position, static_cast<uint32_t>(key >> 32) & 31u, args.base_symbol[position]);
      }
   }
}

/// The four wrappers of one policy: __global__ __launch_bounds__(FOLD_THREADS) functions that call the bodies above.
template <typename Fold>
struct FoldKernels {
   void (*planes)(LayoutArgs, Fold);
   void (*escapes)(LayoutArgs, Fold);
   void (*runs)(LayoutArgs, Fold);
   void (*sparse)(LayoutArgs, Fold);
};

/// Whether the finalized store has a code map, and with it derived symbols and escape keys.
inline bool hasCodeMap(const SeqStoreHost& seqstore) {
   return seqstore.dev.code_map != nullptr && !seqstore.layout.code_map.empty();
}

/// What the plane pass takes an open cell of each position for, into t_base[P]: the position's derived symbol, or NO_SYMBOL.
inline void fillBaseSymbols(const SeqStoreHost& seqstore, uint8_t* t_base) {
   const SeqStoreDev& dev = seqstore.dev;
   uint8_t symbol_of_scan[SCAN_SLOTS];
   std::fill(symbol_of_scan, symbol_of_scan + SCAN_SLOTS, NO_SCAN_SYMBOL);
   for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {
      if (dev.kind[symbol] == PLANE_SCAN && dev.index[symbol] < SCAN_SLOTS) {
         symbol_of_scan[dev.index[symbol]] = static_cast<uint8_t>(symbol);
      }
   }
   const bool has_map = hasCodeMap(seqstore);
   for (uint32_t p = 0; p < dev.positions; ++p) {
      uint32_t base = NO_SYMBOL;
      if (has_map) {
         const uint8_t* map = seqstore.layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
         if ((map[0] & LAYOUT_IMPLICIT) != 0 && map[IMPLICIT_SLOT] < SCAN_SLOTS && symbol_of_scan[map[IMPLICIT_SLOT]] != NO_SCAN_SYMBOL) {
            base = symbol_of_scan[map[IMPLICIT_SLOT]];
         }
      }
      t_base[p] = static_cast<uint8_t>(base);
   }
}

/// The shared arguments of the passes over `seqstore`, with the uploaded base symbols at `base_symbol_dev`.
inline LayoutArgs layoutArgsOf(const silo_gpu_store* store, const SeqStoreHost& seqstore, const uint8_t* base_symbol_dev) {
   const SeqStoreDev& dev = seqstore.dev;
   LayoutArgs args{};
   args.dev = dev;
   args.base_symbol = base_symbol_dev;
   args.sparse_keys = seqstore.d_sparse.get();
   args.n_sparse = seqstore.d_sparse.get() != nullptr ? static_cast<uint32_t>(seqstore.sparse_sorted.size()) : 0u;
   args.n_escapes = hasCodeMap(seqstore) && dev.escapes != nullptr && !seqstore.layout.escape_first.empty() ? seqstore.layout.escape_first.back() : 0u;
   args.sequence_count = store->sequence_count;
   if (dev.extra != nullptr) {
      for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {
         if (dev.kind[symbol] == PLANE_EXTRA && args.n_extra < MAX_EXTRA) {
            args.extra_symbols[args.n_extra++] = static_cast<uint8_t>(symbol);
         }
      }
   }
   return args;
}

/// Builds the two per-position tables — what an open cell of the planes counts as, and the running sums a run of the missing
/// symbol reads — into `scratch_dev` (256-byte aligned, `scratch_bytes` as the entry documents), uploads them, waits for the stream
/// once, and launches the passes the store's layout needs on it without waiting.  `seqstore` is finalized and has planes.
template <typename Fold>
int foldRows(
   const char* entry, const silo_gpu_store* store, const SeqStoreHost& seqstore, void* scratch_dev, size_t scratch_bytes, hipStream_t hip_stream,
   Fold fold, const FoldKernels<Fold>& kernels
) {
   using Value = typename Fold::Value;
   static_assert(sizeof(Value) == 16 && std::is_trivially_copyable<Fold>::value);
   const SeqStoreDev& dev = seqstore.dev;
   HIP_TRY(hipSetDevice(store->device));
   const uint32_t P = dev.positions;

   const size_t base_bytes = align256(P);
   const size_t prefix_bytes = align256((static_cast<size_t>(P) + 1u) * sizeof(Value));
   if (base_bytes + prefix_bytes > scratch_bytes) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": scratch layout exceeds its documented size");  // (cannot happen)
   }
   std::vector<uint8_t> tables(base_bytes + prefix_bytes, 0);
   uint8_t* t_base = tables.data();
   auto* t_prefix = reinterpret_cast<Value*>(tables.data() + base_bytes);
   fillBaseSymbols(seqstore, t_base);
   for (uint32_t p = 0; p < P; ++p) {
      t_prefix[p + 1u] = fold.nextPrefix(t_prefix[p], p, t_base[p], seqstore);
   }
   auto* scratch = static_cast<uint8_t*>(scratch_dev);
   HIP_TRY(hipMemcpyAsync(scratch, tables.data(), tables.size(), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   const LayoutArgs args = layoutArgsOf(store, seqstore, scratch);
   fold.run_prefix = reinterpret_cast<const Value*>(scratch + base_bytes);
   kernels.planes<<<blocksOfWords(dev.row_words, FOLD_WORDS_PER_BLOCK), FOLD_THREADS, 0, hip_stream>>>(args, fold);
   HIP_TRY(hipGetLastError());
   if (args.n_escapes != 0) {
      kernels.escapes<<<strideBlocks(args.n_escapes, FOLD_THREADS), FOLD_THREADS, 0, hip_stream>>>(args, fold);
      HIP_TRY(hipGetLastError());
   }
   if (dev.kind[dev.missing_symbol] == PLANE_RUNS && dev.n_missing_runs != 0 && dev.missing_run_keys != nullptr && dev.missing_run_ends != nullptr) {
      kernels.runs<<<strideBlocks(dev.n_missing_runs, FOLD_THREADS), FOLD_THREADS, 0, hip_stream>>>(args, fold);
      HIP_TRY(hipGetLastError());
   }
   if (args.n_sparse != 0) {
      kernels.sparse<<<strideBlocks(args.n_sparse, FOLD_THREADS), FOLD_THREADS, 0, hip_stream>>>(args, fold);
      HIP_TRY(hipGetLastError());
   }
   return SILO_GPU_OK;
}

/// The store's own copy of such a table: under the store's mutex the first call per sequence store allocates the 16 bytes per
/// row and the scratch, runs `build` (the entry that writes the table) on `stream` and waits; the table and its flag live in
/// `seqstore.*table` and `seqstore.*ready`, and store->device_bytes includes it from then on.
template <typename T>
int keptRowTable(
   const char* entry, silo_gpu_store* store, uint32_t seqstore_id, const T** out_dev, void* stream, DeviceArray<T> SeqStoreHost::*table,
   bool SeqStoreHost::*ready, size_t (*scratch_bytes)(uint32_t positions), int (*build)(const silo_gpu_store*, uint32_t, T*, void*, void*)
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad arguments");
   }
   const std::lock_guard<std::mutex> lock(store->mutex);
   SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (!seqstore.finalized) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": store is not finalized");
   }
   if (!(seqstore.*ready)) {
      HIP_TRY(hipSetDevice(store->device));
      constexpr size_t PER_ROW = 16u / sizeof(T);
      const size_t elements = static_cast<size_t>(seqstore.dev.row_words) * 64u * PER_ROW;
      DeviceArray<T> rows;
      DeviceArray<uint8_t> scratch;
      HIP_TRY(rows.alloc(std::max<size_t>(elements, PER_ROW)));
      HIP_TRY(scratch.alloc(scratch_bytes(seqstore.dev.positions)));
      if (const int status = build(store, seqstore_id, rows.get(), scratch.get(), stream); status != SILO_GPU_OK) {
         (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));  // nothing in flight may outlive the two arrays
         return status;
      }
      HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
      seqstore.*table = std::move(rows);
      seqstore.*ready = true;
      store->device_bytes += elements * sizeof(T);
   }
   *out_dev = (seqstore.*table).get();
   return SILO_GPU_OK;
}

}  // namespace silo_gpu_row_fold
