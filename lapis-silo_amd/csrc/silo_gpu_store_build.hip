// silo_gpu_store_build.hip — the rows of a store coming in: B1 k_transpose_sequences / B2 k_generate_synthetic (aligned sequences ->
// planes, storage/sequence_store.cpp:100-190), in every build mode: the build-time planes, or the counting and the encoding pass of a
// two-pass build with the runs of the missing symbol tracked on the way.  DESIGN.md section 2.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

// ------------------------------------------------------------------------------------------------
// plane writers shared by B1 / B2: `symbol` is this lane's symbol for sequence 64*word+lane
// (SILO_GPU_SYMBOL_NONE contributes no bit).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void emitWord(
   const SeqStoreDev& store, uint32_t position, uint32_t word, uint32_t symbol, bool whole_word,
   uint64_t* sparse, uint32_t* sparse_count, uint32_t sparse_capacity
) {
   const uint32_t lane = threadIdx.x & 63u;
   // valid mutation symbols: the bits of their code go to the bit-sliced scan planes
   const bool is_scan = symbol < store.n_symbols && store.kind[symbol] == PLANE_SCAN;
   const auto put = [&](uint64_t* dst, uint64_t mask) {  // one word of a plane row, by lane 0
      if (mask != 0 && lane == 0) {
         if (whole_word) {
            *dst = mask;
         } else {
            atomicOr(reinterpret_cast<unsigned long long*>(dst), static_cast<unsigned long long>(mask));
         }
      }
   };
   if (store.build_mode == BUILD_COUNT) {  // first pass of a two-pass build: how many rows have which valid symbol here
      const uint32_t scan_index = is_scan ? store.index[symbol] : 0xFFu;
      // ... and how many sparsely stored symbols there are in all (none is stored: the second pass gets a buffer that holds them)
      const uint64_t sparse_lanes = __ballot(symbol < store.n_symbols && store.kind[symbol] == PLANE_SPARSE);
      if (sparse_lanes != 0 && lane == 0) {
         atomicAdd(sparse_count, static_cast<uint32_t>(__popcll(sparse_lanes)));
      }
      for (uint64_t remaining = __ballot(is_scan); remaining != 0;) {
         const uint32_t leader = static_cast<uint32_t>(__builtin_ctzll(remaining));
         const uint32_t leader_index = __shfl(scan_index, leader);
         const uint64_t same = __ballot(is_scan && scan_index == leader_index);
         if (lane == leader) {
            atomicAdd(store.enc_counts + static_cast<size_t>(position) * store.n_scan + leader_index, static_cast<uint32_t>(__popcll(same)));
         }
         remaining &= ~same;
      }
      return;
   }
   if (store.build_mode == BUILD_ENCODE) {  // second pass: straight into the position's adaptive layout
      const uint8_t* map = store.enc_code_map + static_cast<size_t>(position) * CODE_MAP_STRIDE;
      const uint32_t rows_here = map[0] & LAYOUT_ROWS_MASK;
      const bool identity = (map[0] & LAYOUT_IDENTITY) != 0;
      const bool one_hot = (map[0] & LAYOUT_ONE_HOT) != 0;
      const uint32_t scan_index = is_scan ? store.index[symbol] : 0xFFu;
      // the position's derived symbol is stored nowhere: no row, no key
      const bool derived = is_scan && (map[0] & LAYOUT_IMPLICIT) != 0 && map[IMPLICIT_SLOT] == scan_index;
      uint32_t code = 0;  // the code (or 1 + one-hot row) of this lane's symbol here, 0 = not stored
      if (is_scan && !derived) {
         if (identity) {
            code = scan_index + 1u;
         } else {
            const uint32_t n_codes = one_hot ? rows_here + 1u : (1u << rows_here);
            for (uint32_t candidate = 1; candidate < n_codes; ++candidate) {
               code = map[candidate] == scan_index ? candidate : code;
            }
         }
      }
      uint64_t* rows = store.enc_planes + static_cast<size_t>(store.enc_row_of[position]) * store.row_words + word;
      for (uint32_t row = 0; row < rows_here; ++row) {
         put(rows + static_cast<size_t>(row) * store.row_words, __ballot(one_hot ? code == row + 1u : ((code >> row) & 1u) != 0));
      }
      if (is_scan && code == 0 && !derived) {  // a valid symbol the position does not store: an escape key in the symbol's slice of the list
         const size_t counter = static_cast<size_t>(position) * store.n_scan + scan_index;
         const uint32_t slot = store.enc_first[counter] + atomicAdd(store.enc_cursor + counter, 1u);
         if (slot < store.enc_first[counter + 1]) {  // (more rows than the first pass counted: dropped, the cursor tells)
            store.enc_escapes[slot] = (static_cast<uint64_t>(position) << 37) | (static_cast<uint64_t>(scan_index) << 32) | (static_cast<uint64_t>(word) * 64u + lane);
         }
      }
   } else {
      const uint32_t code = is_scan ? static_cast<uint32_t>(store.index[symbol]) + 1u : 0u;
      uint64_t* scan_word = store.scan + static_cast<size_t>(position) * store.n_bits * store.row_words + word;
      for (uint32_t bit = 0; bit < store.n_bits; ++bit) {
         put(scan_word + static_cast<size_t>(bit) * store.row_words, __ballot(((code >> bit) & 1u) != 0));
      }
   }
   // every other symbol: its own plane (extra) or the sorted key list (sparse)
   for (uint32_t s = 0; s < store.n_symbols; ++s) {
      const uint8_t kind = store.kind[s];
      if (kind == PLANE_SCAN) {
         continue;
      }
      const uint64_t mask = __ballot(symbol == s);
      if (mask == 0) {
         continue;
      }
      if (kind == PLANE_EXTRA) {
         if (lane == 0 && store.runs_at_build == 0) {  // (two-pass build: the missing symbol goes to its runs, the kernels track them)
            uint64_t* dst = planePtr(store, position, s) + word;
            if (whole_word) {
               *dst = mask;
            } else {
               atomicOr(reinterpret_cast<unsigned long long*>(dst), static_cast<unsigned long long>(mask));
            }
         }
      } else if (symbol == s) {
         const uint32_t slot = atomicAdd(sparse_count, 1u);
         if (slot < sparse_capacity) {
            sparse[slot] = (static_cast<uint64_t>(position) << 37) | (static_cast<uint64_t>(s) << 32) |
                           (static_cast<uint64_t>(word) * 64u + lane);
         }
      }
   }
}

// ------------------------------------------------------------------------------------------------
// Runs of the missing symbol while a store is built in two passes (SeqStoreDev::runs_at_build): a lane of the build kernels
// walks ONE sequence along the positions of its wave's stretch, so a run is seen from its first to its last position; the
// counting pass counts the runs, the encoding pass writes them (sequence << 32 | start, end) through the same counter.  A
// run that crosses the end of a stretch is listed in pieces — in both passes alike.
// ------------------------------------------------------------------------------------------------
struct MissingRunTracker {
   bool in_run = false;
   uint32_t start = 0;
};

/// Called by every lane of the wave: a run of `sequence` ends at `end` (exclusive) in the lanes where `ends_here`.
__device__ __forceinline__ void emitMissingRun(const SeqStoreDev& store, bool ends_here, uint32_t start, uint32_t end, uint64_t sequence) {
   const uint64_t ending = __ballot(ends_here);
   if (ending == 0) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t leader = static_cast<uint32_t>(__builtin_ctzll(ending));
   unsigned long long first = 0;
   if (lane == leader) {
      first = atomicAdd(store.enc_run_count, static_cast<unsigned long long>(__popcll(ending)));
   }
   if (store.build_mode == BUILD_ENCODE) {
      first = __shfl(first, leader);
      const unsigned long long slot = first + static_cast<unsigned long long>(__popcll(ending & ((1ull << lane) - 1ull)));
      if (ends_here && slot < store.enc_run_capacity) {
         store.enc_run_keys[slot] = (sequence << 32) | start;
         store.enc_run_ends[slot] = end;
      }
   }
}

__device__ __forceinline__ void trackMissingRun(const SeqStoreDev& store, MissingRunTracker& tracker, uint32_t position, bool missing, uint64_t sequence) {
   if (store.runs_at_build == 0) {
      return;
   }
   emitMissingRun(store, tracker.in_run && !missing, tracker.start, position, sequence);
   if (missing && !tracker.in_run) {
      tracker.start = position;
   }
   tracker.in_run = missing;
}

__device__ __forceinline__ void flushMissingRun(const SeqStoreDev& store, MissingRunTracker& tracker, uint32_t end, uint64_t sequence) {
   if (store.runs_at_build != 0) {
      emitMissingRun(store, tracker.in_run, tracker.start, end, sequence);
      tracker.in_run = false;
   }
}

// ------------------------------------------------------------------------------------------------
// B1: transpose a batch of aligned sequences.  A wave owns one 64-sequence word and a range of
// positions; each lane reads 4 positions of its own sequence per load from the pitched staging
// buffer, so consecutive loads of a lane walk the same cache lines.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t TRANSPOSE_POSITIONS_PER_WAVE = 256;

__global__ __launch_bounds__(256) void k_transpose_sequences(
   const SeqStoreDev store,
   const uint8_t* __restrict__ chars,  // [n][pitch]
   const uint8_t* __restrict__ is_null,
   uint32_t pitch,
   uint32_t first_sequence,
   uint32_t n_sequences,
   uint32_t first_word,
   uint32_t n_words,
   const uint8_t* __restrict__ char_table,  // [256]
   uint64_t* sparse,
   uint32_t* sparse_count,
   uint32_t sparse_capacity,
   uint32_t* error_flag
) {
   __shared__ uint8_t s_table[256];
   s_table[threadIdx.x] = char_table[threadIdx.x];
   __syncthreads();

   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t wave_in_block = threadIdx.x >> 6;
   const uint32_t word_index = blockIdx.x * 4 + wave_in_block;
   if (word_index >= n_words) {
      return;
   }
   const uint32_t word = first_word + word_index;
   const uint64_t sequence = static_cast<uint64_t>(word) * 64u + lane;
   const bool active = sequence >= first_sequence && sequence < static_cast<uint64_t>(first_sequence) + n_sequences;
   const uint32_t local = active ? static_cast<uint32_t>(sequence - first_sequence) : 0;
   const bool null_genome = active && is_null != nullptr && is_null[local] != 0;
   // the word is overwritten only if all 64 of its sequences are in this batch
   const bool whole_word = static_cast<uint64_t>(word) * 64u >= first_sequence &&
                           static_cast<uint64_t>(word) * 64u + 64u <= static_cast<uint64_t>(first_sequence) + n_sequences;

   const uint32_t pos_begin = blockIdx.y * TRANSPOSE_POSITIONS_PER_WAVE;
   const uint32_t pos_end = min(store.positions, pos_begin + TRANSPOSE_POSITIONS_PER_WAVE);
   const uint8_t* row = chars + static_cast<size_t>(local) * pitch;
   MissingRunTracker missing_run;
   for (uint32_t p4 = pos_begin; p4 < pos_end; p4 += 4) {
      uint32_t packed = 0;
      if (active && !null_genome) {  // rows are contiguous (pitch = positions, any alignment): byte loads, served from L1
#pragma unroll
         for (uint32_t k = 0; k < 4; ++k) {
            if (p4 + k < pos_end) {
               packed |= static_cast<uint32_t>(row[p4 + k]) << (8 * k);
            }
         }
      }
      for (uint32_t k = 0; k < 4 && p4 + k < pos_end; ++k) {
         uint32_t symbol = SILO_GPU_SYMBOL_NONE;
         if (null_genome) {
            symbol = store.missing_symbol;
         } else if (active) {
            symbol = s_table[(packed >> (8 * k)) & 0xFFu];
            if (symbol == SILO_GPU_SYMBOL_NONE) {
               atomicOr(error_flag, 1u);
            }
         }
         trackMissingRun(store, missing_run, p4 + k, symbol == store.missing_symbol, sequence);
         emitWord(store, p4 + k, word, symbol, whole_word, sparse, sparse_count, sparse_capacity);
      }
   }
   flushMissingRun(store, missing_run, pos_end, sequence);
}

// ------------------------------------------------------------------------------------------------
// B2: synthetic planes (CPU twin: oracle/synth.py symbol_matrix()).
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
   z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
   return z ^ (z >> 31);
}

struct SynthArgs {
   uint64_t seed;
   uint32_t n_lineages;
   uint32_t sequence_count;
   const uint16_t* lineage;
   const uint32_t* lead_gap;
   const uint32_t* trail_gap;
   const uint32_t* missing_start;
   const uint32_t* missing_len;
   const uint8_t* lineage_symbol;  // [P][L]
   const uint8_t* reference;       // [P]
   uint32_t private_threshold;
   uint32_t ambiguous_threshold;
   uint32_t private_base, private_count;      // nuc: 1,4 (A C G T)   aa: 1,20 (A..Y)
   uint32_t ambiguous_base, ambiguous_count;  // nuc: 5,10 (R..V)     aa: 21,2 (B Z)
   uint32_t position_offset;                  // global position of the store's position 0
   uint32_t total_positions;                  // genome length (>= position_offset + store positions)
};

constexpr uint32_t SYNTH_POSITIONS_PER_WAVE = 128;

__global__ __launch_bounds__(256) void k_generate_synthetic(
   const SeqStoreDev store, const SynthArgs args, uint32_t n_words, uint64_t* sparse, uint32_t* sparse_count,
   uint32_t sparse_capacity
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t word = blockIdx.x * 4 + (threadIdx.x >> 6);
   if (word >= n_words) {
      return;
   }
   const uint64_t sequence = static_cast<uint64_t>(word) * 64u + lane;
   const bool active = sequence < args.sequence_count;
   const uint32_t i = active ? static_cast<uint32_t>(sequence) : 0;
   const uint32_t lineage = args.lineage[i];
   const uint32_t lead = args.lead_gap[i];
   const uint32_t trail = args.trail_gap[i];
   const uint32_t mstart = args.missing_start[i];
   const uint32_t mlen = args.missing_len[i];
   const uint32_t positions = args.total_positions;
   const uint64_t seq_hash = args.seed ^ (static_cast<uint64_t>(i) * 0x9E3779B97F4A7C15ull);

   const uint32_t pos_begin = blockIdx.y * SYNTH_POSITIONS_PER_WAVE;
   const uint32_t pos_end = min(store.positions, pos_begin + SYNTH_POSITIONS_PER_WAVE);
   MissingRunTracker missing_run;
   for (uint32_t local = pos_begin; local < pos_end; ++local) {
      const uint32_t p = args.position_offset + local;  // global genome position
      uint32_t symbol;
      if (p < lead || p >= positions - trail) {
         symbol = 0;  // GAP
      } else if (p >= mstart && p - mstart < mlen) {
         symbol = store.missing_symbol;
      } else {
         const uint64_t h = mix64(seq_hash ^ (static_cast<uint64_t>(p) * 0xC2B2AE3D27D4EB4Full));
         if ((h & 0xFFFFFu) < args.private_threshold) {
            symbol = args.private_base + static_cast<uint32_t>((h >> 20) & 0xFFFu) % args.private_count;
         } else if (((h >> 32) & 0xFFFFFFu) < args.ambiguous_threshold) {
            symbol = args.ambiguous_base + static_cast<uint32_t>(h >> 56) % args.ambiguous_count;
         } else {
            const uint8_t ls = args.lineage_symbol[static_cast<size_t>(local) * args.n_lineages + lineage];
            symbol = ls != SILO_GPU_SYMBOL_NONE ? ls : args.reference[local];
         }
      }
      if (!active) {
         symbol = SILO_GPU_SYMBOL_NONE;
      }
      trackMissingRun(store, missing_run, local, symbol == store.missing_symbol, sequence);
      emitWord(store, local, word, symbol, /*whole_word=*/true, sparse, sparse_count, sparse_capacity);
   }
   flushMissingRun(store, missing_run, pos_end, sequence);
}

/// Runs a build kernel over a batch: `launch(sparse_capacity)` enqueues it with the sparse buffer as it is now.
/// The dense writes of an ordinary build are idempotent (atomicOr / whole-word stores); if the sparse buffer overflows the counter
/// is rewound to `rewind_to`, the buffer grown and the batch replayed, `attempts` times at the most.
/// The passes of a two-pass build must not be replayed — the counting pass adds to counters, the encoding pass takes key slots
/// and run slots with atomic cursors — so they never overflow the sparse buffer: the counting pass stores no sparse key at all
/// (capacity 0: the counter counts them), silo_gpu_store_build_pass(2) sizes the buffer from that count.
template <typename Launch>
int launchAndReplay(SeqStoreHost& seqstore, uint32_t rewind_to, uint32_t reserve, int attempts, const char* kernel, Launch launch) {
   const uint32_t build_mode = seqstore.dev.build_mode;
   if (build_mode == BUILD_PLANES) {
      if (int rc = growSparse(seqstore, reserve); rc != SILO_GPU_OK) {
         return rc;
      }
   }
   for (int attempt = 0; attempt < attempts; ++attempt) {
      launch(build_mode == BUILD_COUNT ? 0u : seqstore.sparse_capacity);
      hipError_t err = hipDeviceSynchronize();
      uint32_t count_after = 0;
      if (err == hipSuccess) {
         err = hipMemcpy(&count_after, seqstore.d_sparse_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost);
      }
      if (err != hipSuccess) {
         return fail(SILO_GPU_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(err));
      }
      if (build_mode == BUILD_COUNT || count_after <= seqstore.sparse_capacity) {
         break;
      }
      if (build_mode == BUILD_ENCODE) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "two-pass build: the second pass brought more sparsely stored symbols than the first pass counted");
      }
      err = hipMemcpy(seqstore.d_sparse_count.get(), &rewind_to, sizeof(uint32_t), hipMemcpyHostToDevice);
      if (err != hipSuccess) {
         return fail(SILO_GPU_ERR_HIP, std::string("rewinding sparse counter: ") + hipGetErrorString(err));
      }
      if (int rc = growSparse(seqstore, count_after); rc != SILO_GPU_OK) {
         return rc;
      }
   }
   return SILO_GPU_OK;
}

}  // namespace

extern "C" {

int silo_gpu_store_append_sequences(
   silo_gpu_store* store, uint32_t seqstore_id, uint32_t first_sequence, uint32_t n_sequences, const char* chars,
   const uint8_t* is_null
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || (chars == nullptr && n_sequences > 0)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_append_sequences: bad arguments");
   }
   if (static_cast<uint64_t>(first_sequence) + n_sequences > store->sequence_count) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "append beyond sequence_count");
   }
   if (n_sequences == 0) {
      return SILO_GPU_OK;
   }
   std::lock_guard<std::mutex> lock(store->mutex);
   HIP_TRY(hipSetDevice(store->device));
   SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (const int rc = ensureBuildPlanes(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   seqstore.finalized = false;
   seqstore.totals_ready = seqstore.dev.build_mode == BUILD_ENCODE;  // (the counts of the first pass ARE the totals)
   if (seqstore.dev.build_mode != BUILD_ENCODE) {
      seqstore.rows_filled += n_sequences;
   }
   const uint32_t positions = seqstore.dev.positions;
   const uint32_t pitch = positions;  // rows stay contiguous: ONE host-to-device copy per batch

   const size_t stage_bytes = static_cast<size_t>(n_sequences) * pitch;
   if (stage_bytes > store->stage_capacity) {
      store->stage_capacity = 0;
      HIP_TRY(store->d_stage.alloc(stage_bytes));
      store->stage_capacity = stage_bytes;
   }
   if (is_null != nullptr && n_sequences > store->stage_null_capacity) {
      store->stage_null_capacity = 0;
      HIP_TRY(store->d_stage_null.alloc(n_sequences));
      store->stage_null_capacity = n_sequences;
   }
   DeviceArray<uint8_t>& d_table_slot = store->d_char_table[seqstore.alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE ? 0 : 1];
   if (d_table_slot.get() == nullptr) {
      uint8_t table[256];
      fillCharTable(seqstore.alphabet, table);
      DeviceArray<uint8_t> uploaded;
      HIP_TRY(uploaded.alloc(256));
      HIP_TRY(hipMemcpy(uploaded.get(), table, 256, hipMemcpyHostToDevice));
      d_table_slot = std::move(uploaded);
   }
   uint8_t* d_chars = store->d_stage.get();
   uint8_t* d_null = is_null != nullptr ? store->d_stage_null.get() : nullptr;
   uint8_t* d_table = d_table_slot.get();
   HIP_TRY(hipMemcpy(d_chars, chars, stage_bytes, hipMemcpyHostToDevice));
   if (is_null != nullptr) {
      HIP_TRY(hipMemcpy(d_null, is_null, n_sequences, hipMemcpyHostToDevice));
   }

   const uint32_t first_word = first_sequence / 64u;
   const uint32_t last_word = (first_sequence + n_sequences - 1u) / 64u;
   const uint32_t n_words = last_word - first_word + 1u;
   const dim3 grid((n_words + 3) / 4, (positions + TRANSPOSE_POSITIONS_PER_WAVE - 1) / TRANSPOSE_POSITIONS_PER_WAVE);

   uint32_t count_before = 0;
   const hipError_t err = hipMemcpy(&count_before, seqstore.d_sparse_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost);
   if (err != hipSuccess) {
      return fail(SILO_GPU_ERR_HIP, std::string("reading sparse counter: ") + hipGetErrorString(err));
   }
   const int rc = launchAndReplay(seqstore, count_before, count_before + (1u << 16), 8, "k_transpose_sequences", [&](uint32_t sparse_capacity) {
      k_transpose_sequences<<<grid, 256>>>(
         seqstore.dev, d_chars, d_null, pitch, first_sequence, n_sequences, first_word, n_words, d_table,
         seqstore.d_sparse.get(), seqstore.d_sparse_count.get(), sparse_capacity, store->d_error_flag.get()
      );
   });
   if (rc != SILO_GPU_OK) {
      return rc;
   }
   uint32_t error_flag = 0;
   HIP_TRY(hipMemcpy(&error_flag, store->d_error_flag.get(), sizeof(uint32_t), hipMemcpyDeviceToHost));
   if (error_flag != 0) {
      HIP_TRY(hipMemset(store->d_error_flag.get(), 0, sizeof(uint32_t)));
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "Illegal character contained in sequence.");
   }
   return SILO_GPU_OK;
}

int silo_gpu_store_generate_synthetic(silo_gpu_store* store, uint32_t seqstore_id, const silo_gpu_synth_desc* synth) {
   if (store == nullptr || synth == nullptr || seqstore_id >= store->seqstores.size() || synth->n_lineages == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_generate_synthetic: bad arguments");
   }
   std::lock_guard<std::mutex> lock(store->mutex);
   HIP_TRY(hipSetDevice(store->device));
   SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   if (const int rc = ensureBuildPlanes(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   seqstore.finalized = false;
   seqstore.totals_ready = seqstore.dev.build_mode == BUILD_ENCODE;
   seqstore.rows_filled = store->sequence_count;
   const uint32_t n = store->sequence_count;
   const uint32_t positions = seqstore.dev.positions;

   DeviceArray<uint32_t> d_u32[4];
   DeviceArray<uint8_t> d_lineage_symbol;
   hipError_t err = hipSuccess;
   if (store->d_lineage.get() == nullptr) {
      err = store->d_lineage.alloc(n);
   }
   if (err == hipSuccess) {
      err = hipMemcpy(store->d_lineage.get(), synth->lineage_of_sequence, static_cast<size_t>(n) * sizeof(uint16_t), hipMemcpyHostToDevice);
      store->n_lineages = synth->n_lineages;
   }
   const uint32_t* host_u32[4] = {synth->lead_gap, synth->trail_gap, synth->missing_start, synth->missing_len};
   for (int k = 0; k < 4 && err == hipSuccess; ++k) {
      err = d_u32[k].alloc(n);
      if (err == hipSuccess) {
         err = hipMemcpy(d_u32[k].get(), host_u32[k], static_cast<size_t>(n) * sizeof(uint32_t), hipMemcpyHostToDevice);
      }
   }
   const size_t table_bytes = static_cast<size_t>(positions) * synth->n_lineages;
   if (err == hipSuccess) {
      err = d_lineage_symbol.alloc(table_bytes);
   }
   if (err == hipSuccess) {
      err = hipMemcpy(d_lineage_symbol.get(), synth->lineage_symbol, table_bytes, hipMemcpyHostToDevice);
   }
   if (err != hipSuccess) {
      return fail(SILO_GPU_ERR_HIP, std::string("staging synthetic model: ") + hipGetErrorString(err));
   }

   SynthArgs args{};
   args.seed = synth->seed;
   args.n_lineages = synth->n_lineages;
   args.sequence_count = n;
   args.lineage = store->d_lineage.get();
   args.lead_gap = d_u32[0].get();
   args.trail_gap = d_u32[1].get();
   args.missing_start = d_u32[2].get();
   args.missing_len = d_u32[3].get();
   args.lineage_symbol = d_lineage_symbol.get();
   args.reference = seqstore.d_reference.get();
   args.private_threshold = synth->private_threshold;
   args.ambiguous_threshold = synth->ambiguous_threshold;
   args.position_offset = synth->position_offset;
   args.total_positions = synth->total_positions != 0 ? synth->total_positions : positions;
   if (static_cast<uint64_t>(args.position_offset) + positions > args.total_positions) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "synthetic position window exceeds total_positions");
   }
   if (seqstore.alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      args.private_base = 1;
      args.private_count = 4;
      args.ambiguous_base = 5;
      args.ambiguous_count = 10;
   } else {
      args.private_base = 1;
      args.private_count = 20;
      args.ambiguous_base = 21;
      args.ambiguous_count = 2;
   }

   const uint32_t n_words = (n + 63u) / 64u;
   const dim3 grid((n_words + 3) / 4, (positions + SYNTH_POSITIONS_PER_WAVE - 1) / SYNTH_POSITIONS_PER_WAVE);
   // expected sparse entries: cells * ambiguous_threshold / 2^24 (+ slack)
   const double expected = static_cast<double>(n) * positions * (static_cast<double>(synth->ambiguous_threshold) / 16777216.0);
   uint32_t zero = 0;
   err = hipMemcpy(seqstore.d_sparse_count.get(), &zero, sizeof(uint32_t), hipMemcpyHostToDevice);
   if (err != hipSuccess) {
      return fail(SILO_GPU_ERR_HIP, std::string("resetting sparse counter: ") + hipGetErrorString(err));
   }
   const double wanted = expected * 1.25 + 65536.0;
   if (wanted > 4.0e9) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "ambiguous_threshold too large for the sparse store");
   }
   return launchAndReplay(seqstore, 0u, static_cast<uint32_t>(wanted), 4, "k_generate_synthetic", [&](uint32_t sparse_capacity) {
      k_generate_synthetic<<<grid, 256>>>(seqstore.dev, args, n_words, seqstore.d_sparse.get(), seqstore.d_sparse_count.get(), sparse_capacity);
   });
}

}  // extern "C"
