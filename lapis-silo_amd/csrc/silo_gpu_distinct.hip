// silo_gpu_distinct.hip — K20, the filter expression DistinctSequences: a 128-bit hash of every row of a sequence
// store (row_hash.h), kept by the store, and a hash-table pass over the selected rows of any number of partitions that leaves one
// row — the one with the smallest number in the database — per class of rows with equal hashes.
// The hashes are read off the store's layout with the decomposition of K11 (silo_gpu_nearest.hip): every row gets the terms of what
// the planes say, and each stored thing beside the planes corrects its cell with the difference of two terms, mod 2^64:
//   k_row_hash_planes    a wave per row word, a lane per row, all positions: the lane's code at the position (code planes, one-hot
//                        rows, extra planes) selects the symbol, an open cell counts as the position's derived symbol or as 31;
//                        the two sums stay in registers and leave with one 16-byte store per row ((0, 0) for padding rows)
//   k_row_hash_escapes   a thread per escape key: H(p, its symbol) - H(p, what the planes said)
//   k_row_hash_runs      a thread per run [a, e) of the missing symbol: two lookups in a prefix array of those differences
//   k_row_hash_sparse    a thread per sparse key (ambiguity code)
// The selection, on row bitsets and arrays of hashes, takes no store (what it shares with the class counts of K21 — the hash of a
// global row, the load of an owner, the refusals — is in distinct_table.h):
//   k_distinct_begin     every slot of the owner table empty, the overflow counter 0
//   k_distinct_insert    a wave per filter word, a lane per selected row: linear probing with compare-and-swap / atomic min
//   k_distinct_select    a thread per row, a wave's ballot per word: the rows that own their class's slot
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "distinct_table.h"
#include "row_hash.h"
#include "store_internal.h"

using namespace silo_gpu_detail;
using namespace silo_gpu_distinct_table;
using silo_gpu_row_hash::NO_SYMBOL;
using silo_gpu_row_hash::term;

namespace {

constexpr uint32_t MAX_EXTRA = 16;
constexpr uint32_t SCAN_SLOTS = 32;  // scan symbol indices a key can name (5 bits)
constexpr uint8_t NO_SCAN_SYMBOL = 0xFF;
static_assert(NO_SYMBOL == SILO_GPU_ROW_HASH_NO_SYMBOL && NO_SYMBOL >= SILO_GPU_MAX_SYMBOLS && NO_SYMBOL < 32u);

struct HashArgs {
   SeqStoreDev dev;
   const uint8_t* base_symbol;   // [P] what the plane pass takes an open cell for: the derived symbol, or NO_SYMBOL
   const uint64_t* run_prefix;   // [P + 1][2] sums over q < p of H(q, missing symbol) - H(q, base_symbol[q])
   const uint64_t* sparse_keys;
   uint32_t n_sparse;
   uint32_t n_escapes;
   uint32_t sequence_count;
   uint32_t n_extra;
   uint8_t extra_symbols[MAX_EXTRA];  // symbols kept in extra planes
   uint64_t* out;                // [row_words * 64][2]
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

/// grid = row_words / WORDS_PER_BLOCK rounded up.  The plane words of a position are loaded once per wave (the address is uniform)
/// and every lane takes its own bit of them.
__global__ __launch_bounds__(THREADS) void k_row_hash_planes(const HashArgs args) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   const uint32_t row_words = args.dev.row_words;
   const uint32_t word = blockIdx.x * WORDS_PER_BLOCK + (threadIdx.x >> 6);  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t n_scan = args.dev.n_scan;
   const bool has_extra = args.n_extra != 0 && args.dev.extra != nullptr;
   uint64_t h0 = 0, h1 = 0;
   for (uint32_t position = 0; position < args.dev.positions; ++position) {
      const PositionLayout layout = layoutOf(args.dev, position);
      uint32_t code = 0;
      for (uint32_t plane = 0; plane < layout.bits; ++plane) {
         const uint32_t set = static_cast<uint32_t>((layout.rows[static_cast<size_t>(plane) * row_words + word] >> lane) & 1ull);
         code = layout.one_hot ? (set != 0 ? plane + 1u : code) : (code | (set << plane));
      }
      uint32_t symbol = args.base_symbol[position];
      if (code != 0) {
         const uint32_t scan_index = layout.identity ? code - 1u : (code < CODE_MAP_STRIDE ? layout.map[code] : NO_SCAN_SYMBOL);
         if (scan_index < n_scan && scan_index < SCAN_SLOTS) {
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
      h0 += term(position, symbol, 0);
      h1 += term(position, symbol, 1);
   }
   const uint64_t row = static_cast<uint64_t>(word) * 64u + lane;
   const bool real = row < args.sequence_count;
   reinterpret_cast<ulonglong2*>(args.out)[row] = real ? make_ulonglong2(h0, h1) : make_ulonglong2(0ull, 0ull);
}

/// Adds H(position, symbol) - H(position, base) to the row's cell, lane by lane.
__device__ __forceinline__ void correct(const HashArgs& args, uint32_t row, uint32_t position, uint32_t symbol) {
   const uint32_t base = args.base_symbol[position];
   if (symbol == base) {
      return;
   }
   auto* cell = reinterpret_cast<unsigned long long*>(args.out) + 2u * static_cast<size_t>(row);
   atomicAdd(cell, static_cast<unsigned long long>(term(position, symbol, 0) - term(position, base, 0)));
   atomicAdd(cell + 1, static_cast<unsigned long long>(term(position, symbol, 1) - term(position, base, 1)));
}

/// A thread per escape key (grid-stride): a row's valid symbol that has neither a code nor a row at its position.
__global__ __launch_bounds__(THREADS) void k_row_hash_escapes(const HashArgs args) {
   __shared__ uint8_t s_symbol_of_scan[SCAN_SLOTS];
   fillSymbolOfScan(s_symbol_of_scan, args.dev);
   for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < args.n_escapes; i += gridDim.x * THREADS) {
      const uint64_t key = args.dev.escapes[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t symbol = s_symbol_of_scan[static_cast<uint32_t>(key >> 32) & 31u];
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count && symbol != NO_SCAN_SYMBOL) {
         correct(args, row, position, symbol);
      }
   }
}

/// A thread per run of the missing symbol (grid-stride).
__global__ __launch_bounds__(THREADS) void k_row_hash_runs(const HashArgs args) {
   for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < args.dev.n_missing_runs; i += gridDim.x * THREADS) {
      const uint64_t key = args.dev.missing_run_keys[i];
      const uint32_t row = static_cast<uint32_t>(key >> 32);
      const uint32_t start = static_cast<uint32_t>(key);
      const uint32_t end = min(args.dev.missing_run_ends[i], args.dev.positions);
      if (start < end && row < args.sequence_count) {
         auto* cell = reinterpret_cast<unsigned long long*>(args.out) + 2u * static_cast<size_t>(row);
         const uint64_t d0 = args.run_prefix[2u * static_cast<size_t>(end)] - args.run_prefix[2u * static_cast<size_t>(start)];
         const uint64_t d1 = args.run_prefix[2u * static_cast<size_t>(end) + 1u] - args.run_prefix[2u * static_cast<size_t>(start) + 1u];
         atomicAdd(cell, static_cast<unsigned long long>(d0));
         atomicAdd(cell + 1, static_cast<unsigned long long>(d1));
      }
   }
}

/// A thread per sparse key (grid-stride): an ambiguity code, or the missing symbol where it has neither runs nor a plane.
__global__ __launch_bounds__(THREADS) void k_row_hash_sparse(const HashArgs args) {
   for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < args.n_sparse; i += gridDim.x * THREADS) {
      const uint64_t key = args.sparse_keys[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t row = static_cast<uint32_t>(key);
      if (position < args.dev.positions && row < args.sequence_count) {
         correct(args, row, position, static_cast<uint32_t>(key >> 32) & 31u);
      }
   }
}

size_t align256(size_t bytes) {
   return (bytes + 255u) / 256u * 256u;
}

uint32_t strideBlocks(uint32_t items) {
   return std::min<uint32_t>((items + THREADS - 1u) / THREADS, 4096u);
}

// ---- the selection ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_distinct_begin(uint32_t* __restrict__ table, uint32_t slots) {
   const uint64_t word = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
   if (word <= slots) {
      table[word] = word == slots ? 0u : EMPTY;  // the overflow counter sits behind the slots
   }
}

/// grid <= MAX_WALK_BLOCKS; a wave takes the filter words wave, wave + waves of the grid, ...  No lane waits for another: every
/// step of the probe is one atomic whose outcome is final for that slot's class.
__global__ __launch_bounds__(THREADS) void k_distinct_insert(
   uint32_t* __restrict__ table, uint32_t slots, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, uint32_t part,
   const uint64_t* __restrict__ filter
) {
   const silo_gpu_distinct_part mine = parts[part];
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t mask = slots - 1u;
   const uint64_t step = static_cast<uint64_t>(gridDim.x) * WORDS_PER_BLOCK;
   for (uint64_t word = static_cast<uint64_t>(blockIdx.x) * WORDS_PER_BLOCK + (threadIdx.x >> 6); word < mine.row_words; word += step) {
      const uint64_t bits = filter[word];
      const uint64_t row = word * 64u + lane;
      if (((bits >> lane) & 1ull) == 0 || row >= mine.sequence_count) {
         continue;
      }
      const ulonglong2 hash = reinterpret_cast<const ulonglong2*>(mine.hashes_dev)[row];
      const uint32_t g = mine.first_row + static_cast<uint32_t>(row);
      uint32_t slot = static_cast<uint32_t>(hash.x) & mask;
      bool placed = false;
      for (uint32_t probes = 0; probes < slots && !placed; ++probes) {
         uint32_t owner = loadOwner(table + slot);
         if (owner == EMPTY) {
            owner = atomicCAS(table + slot, EMPTY, g);
            if (owner == EMPTY) {
               placed = true;
               break;
            }
         }
         if (owner == g) {
            placed = true;
            break;
         }
         const ulonglong2 other = hashOfGlobalRow(parts, n_parts, owner);
         if (other.x == hash.x && other.y == hash.y) {
            if (g < owner) {
               atomicMin(table + slot, g);
            }
            placed = true;
            break;
         }
         slot = (slot + 1u) & mask;
      }
      if (!placed) {
         atomicAdd(table + slots, 1u);
      }
   }
}

/// A thread per row, a wave per word of the output: a wave whose word is at or past row_words neither loads nor stores.
__global__ __launch_bounds__(THREADS) void k_distinct_select(
   const uint32_t* __restrict__ table, uint32_t slots, const silo_gpu_distinct_part* __restrict__ parts, uint32_t n_parts, uint32_t part,
   const uint64_t* __restrict__ filter, uint64_t* __restrict__ out
) {
   const silo_gpu_distinct_part mine = parts[part];
   const uint64_t row = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
   const uint64_t word = row >> 6;  // (uniform over the wave)
   if (word >= mine.row_words) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t bits = filter[word];
   bool selected = false;
   if (((bits >> lane) & 1ull) != 0 && row < mine.sequence_count) {
      const ulonglong2 hash = reinterpret_cast<const ulonglong2*>(mine.hashes_dev)[row];
      const uint32_t g = mine.first_row + static_cast<uint32_t>(row);
      const uint32_t mask = slots - 1u;
      uint32_t slot = static_cast<uint32_t>(hash.x) & mask;
      for (uint32_t probes = 0; probes < slots; ++probes) {
         const uint32_t owner = table[slot];
         if (owner == EMPTY) {
            break;  // (a row that was never inserted)
         }
         if (owner == g) {
            selected = true;
            break;
         }
         const ulonglong2 other = hashOfGlobalRow(parts, n_parts, owner);
         if (other.x == hash.x && other.y == hash.y) {
            break;  // its class is represented by an earlier row
         }
         slot = (slot + 1u) & mask;
      }
   }
   const uint64_t ballot = __ballot(selected);
   if (lane == 0) {
      out[word] = ballot;
   }
}

}  // namespace

extern "C" {

uint64_t silo_gpu_row_hash_term(uint32_t position, uint32_t symbol, uint32_t lane) {
   return term(position, symbol, lane != 0 ? 1u : 0u);
}

int silo_gpu_row_hashes(const silo_gpu_store* store, uint32_t seqstore_id, uint64_t* out_dev, void* scratch_dev, void* stream) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_hashes: bad arguments");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (!seqstore.finalized || dev.planes == nullptr || dev.row_words == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_hashes: store is not finalized");
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);
   const uint32_t P = dev.positions;

   // the per-position tables: what an open cell of the planes counts as, and the running sums a run of the missing symbol reads
   uint8_t symbol_of_scan[SCAN_SLOTS];
   std::fill(symbol_of_scan, symbol_of_scan + SCAN_SLOTS, NO_SCAN_SYMBOL);
   for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {
      if (dev.kind[symbol] == PLANE_SCAN && dev.index[symbol] < SCAN_SLOTS) {
         symbol_of_scan[dev.index[symbol]] = static_cast<uint8_t>(symbol);
      }
   }
   const bool has_map = dev.code_map != nullptr && !seqstore.layout.code_map.empty();
   const size_t base_bytes = align256(P);
   const size_t prefix_bytes = align256((static_cast<size_t>(P) + 1u) * 2u * sizeof(uint64_t));
   if (base_bytes + prefix_bytes > SILO_GPU_ROW_HASH_SCRATCH_BYTES(P)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_row_hashes: scratch layout exceeds its documented size");  // (cannot happen)
   }
   std::vector<uint8_t> tables(base_bytes + prefix_bytes, 0);
   uint8_t* t_base = tables.data();
   auto* t_prefix = reinterpret_cast<uint64_t*>(tables.data() + base_bytes);
   const uint32_t missing = dev.missing_symbol;
   for (uint32_t p = 0; p < P; ++p) {
      uint32_t base = NO_SYMBOL;
      if (has_map) {
         const uint8_t* map = seqstore.layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
         if ((map[0] & LAYOUT_IMPLICIT) != 0 && map[IMPLICIT_SLOT] < SCAN_SLOTS && symbol_of_scan[map[IMPLICIT_SLOT]] != NO_SCAN_SYMBOL) {
            base = symbol_of_scan[map[IMPLICIT_SLOT]];
         }
      }
      t_base[p] = static_cast<uint8_t>(base);
      t_prefix[2u * (p + 1u)] = t_prefix[2u * p] + (term(p, missing, 0) - term(p, base, 0));
      t_prefix[2u * (p + 1u) + 1u] = t_prefix[2u * p + 1u] + (term(p, missing, 1) - term(p, base, 1));
   }
   auto* scratch = static_cast<uint8_t*>(scratch_dev);
   HIP_TRY(hipMemcpyAsync(scratch, tables.data(), tables.size(), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   HashArgs args{};
   args.dev = dev;
   args.base_symbol = scratch;
   args.run_prefix = reinterpret_cast<const uint64_t*>(scratch + base_bytes);
   args.sparse_keys = seqstore.d_sparse.get();
   args.n_sparse = seqstore.d_sparse.get() != nullptr ? static_cast<uint32_t>(seqstore.sparse_sorted.size()) : 0u;
   args.n_escapes = has_map && dev.escapes != nullptr && !seqstore.layout.escape_first.empty() ? seqstore.layout.escape_first.back() : 0u;
   args.sequence_count = store->sequence_count;
   args.out = out_dev;
   if (dev.extra != nullptr) {
      for (uint32_t symbol = 0; symbol < dev.n_symbols; ++symbol) {
         if (dev.kind[symbol] == PLANE_EXTRA && args.n_extra < MAX_EXTRA) {
            args.extra_symbols[args.n_extra++] = static_cast<uint8_t>(symbol);
         }
      }
   }
   k_row_hash_planes<<<blocksOfWords(dev.row_words), THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   if (args.n_escapes != 0) {
      k_row_hash_escapes<<<strideBlocks(args.n_escapes), THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (dev.kind[missing] == PLANE_RUNS && dev.n_missing_runs != 0 && dev.missing_run_keys != nullptr && dev.missing_run_ends != nullptr) {
      k_row_hash_runs<<<strideBlocks(dev.n_missing_runs), THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (args.n_sparse != 0) {
      k_row_hash_sparse<<<strideBlocks(args.n_sparse), THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   return SILO_GPU_OK;
}

int silo_gpu_store_row_hashes(silo_gpu_store* store, uint32_t seqstore_id, const uint64_t** out_dev, void* stream) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_row_hashes: bad arguments");
   }
   const std::lock_guard<std::mutex> lock(store->mutex);
   SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (!seqstore.finalized) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_row_hashes: store is not finalized");
   }
   if (!seqstore.row_hashes_ready) {
      HIP_TRY(hipSetDevice(store->device));
      const size_t words = static_cast<size_t>(seqstore.dev.row_words) * 64u * 2u;
      DeviceArray<uint64_t> hashes;
      DeviceArray<uint8_t> scratch;
      HIP_TRY(hashes.alloc(std::max<size_t>(words, 2u)));
      HIP_TRY(scratch.alloc(SILO_GPU_ROW_HASH_SCRATCH_BYTES(seqstore.dev.positions)));
      if (const int status = silo_gpu_row_hashes(store, seqstore_id, hashes.get(), scratch.get(), stream); status != SILO_GPU_OK) {
         (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));  // nothing in flight may outlive the two arrays
         return status;
      }
      HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
      seqstore.d_row_hashes = std::move(hashes);
      seqstore.row_hashes_ready = true;
      store->device_bytes += words * sizeof(uint64_t);
   }
   *out_dev = seqstore.d_row_hashes.get();
   return SILO_GPU_OK;
}

int silo_gpu_distinct_begin(void* table_dev, uint32_t slots, void* stream) {
   if (table_dev == nullptr || slots == 0 || (slots & (slots - 1u)) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_distinct_begin: no table, or slots is not a power of two");
   }
   const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(slots) + 1u + THREADS - 1u) / THREADS);
   k_distinct_begin<<<blocks, THREADS, 0, static_cast<hipStream_t>(stream)>>>(static_cast<uint32_t*>(table_dev), slots);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distinct_insert(
   void* table_dev, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part, const uint64_t* filter_dev,
   void* stream
) {
   auto hip_stream = static_cast<hipStream_t>(stream);
   silo_gpu_distinct_part mine{};
   if (const int status = checkSelection("silo_gpu_distinct_insert", table_dev, slots, parts_dev, n_parts, part, filter_dev, table_dev, hip_stream, mine);
       status != SILO_GPU_OK) {
      return status;
   }
   k_distinct_insert<<<std::min(blocksOfWords(mine.row_words), MAX_WALK_BLOCKS), THREADS, 0, hip_stream>>>(
      static_cast<uint32_t*>(table_dev), slots, parts_dev, n_parts, part, filter_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distinct_select(
   const void* table_dev, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, uint64_t* out_bitset_dev, void* stream
) {
   auto hip_stream = static_cast<hipStream_t>(stream);
   silo_gpu_distinct_part mine{};
   if (const int status = checkSelection("silo_gpu_distinct_select", table_dev, slots, parts_dev, n_parts, part, filter_dev, out_bitset_dev, hip_stream, mine);
       status != SILO_GPU_OK) {
      return status;
   }
   k_distinct_select<<<blocksOfWords(mine.row_words), THREADS, 0, hip_stream>>>(
      static_cast<const uint32_t*>(table_dev), slots, parts_dev, n_parts, part, filter_dev, out_bitset_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
