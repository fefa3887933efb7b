// silo_gpu_store_streams.hip — what finalize derives from a store for the scan: the runs of the missing symbol and their slice index,
// the slice-major packed streams (escape keys, gap events, end events, residual keys), the bounds a pruning scan reads.  DESIGN.md
// sections 3 and 4.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_internal.h"

using namespace silo_gpu_detail;

using silo_gpu_layout::KEY_COST_BYTES;

namespace {

/// The slice-major keys as k_scan_escapes_sliced reads them (SeqStoreHost::Layout::escapes_sliced): one block per granule of
/// ESCAPE_GRANULE_KEYS keys of one slice.  `unpacked_first[g]` = index of the granule's first key in the sorted 8-byte list,
/// `unpacked_end[g]` = one past its last (a slice's last granule is short: the rest is padding).
__global__ __launch_bounds__(256) void k_pack_sliced_keys(
   const uint64_t* __restrict__ keys, const uint32_t* __restrict__ unpacked_first, const uint32_t* __restrict__ unpacked_end, uint32_t n_scan,
   uint32_t* __restrict__ packed, uint32_t* __restrict__ granule_base, uint64_t* __restrict__ overflow, uint32_t* __restrict__ overflow_count,
   uint32_t overflow_capacity
) {
   const uint32_t granule = blockIdx.x;
   const uint32_t begin = unpacked_first[granule];
   const uint32_t end = unpacked_end[granule];
   const auto counter_of = [n_scan](uint64_t key) { return static_cast<uint32_t>(key >> 37) * n_scan + (static_cast<uint32_t>(key >> 32) & 31u); };
   const uint32_t base = begin < end ? counter_of(keys[begin]) : 0u;
   if (threadIdx.x == 0) {
      granule_base[granule] = base;
   }
   for (uint32_t k = threadIdx.x; k < ESCAPE_GRANULE_KEYS; k += blockDim.x) {
      uint32_t value = ESCAPE_KEY_INVALID;
      if (begin + k < end) {
         const uint64_t key = keys[begin + k];
         const uint32_t relative = counter_of(key) - base;
         if (relative <= ESCAPE_MAX_RELATIVE) {
            value = (relative << ESCAPE_SLICE_SHIFT) | (static_cast<uint32_t>(key) & ESCAPE_ROW_MASK);
         } else {
            const uint32_t slot = atomicAdd(overflow_count, 1u);
            if (slot < overflow_capacity) {
               overflow[slot] = (static_cast<uint64_t>(counter_of(key)) << 32) | (key & 0xFFFFFFFFull);
            }
         }
      }
      packed[static_cast<size_t>(granule) * ESCAPE_GRANULE_KEYS + k] = value;
   }
}

/// first[slice][p] = index of the first slice-major key of (slice, position >= p): a binary search per entry.
__global__ __launch_bounds__(256) void k_slice_index(
   const uint64_t* __restrict__ keys, uint32_t n_keys, uint32_t slice_shift, uint32_t n_slices, uint32_t positions, uint32_t* __restrict__ first
) {
   const uint32_t entry = blockIdx.x * blockDim.x + threadIdx.x;
   if (entry >= n_slices * (positions + 1u)) {
      return;
   }
   const uint32_t slice = entry / (positions + 1u);
   const uint32_t position = entry % (positions + 1u);
   uint32_t lo = 0, hi = n_keys;
   while (lo < hi) {  // keys before (slice, position): a smaller slice, or the same slice and a smaller position
      const uint32_t mid = lo + (hi - lo) / 2;
      const uint32_t key_slice = static_cast<uint32_t>(keys[mid]) >> slice_shift;
      const uint32_t key_position = static_cast<uint32_t>(keys[mid] >> 37);
      if (key_slice < slice || (key_slice == slice && key_position < position)) {
         lo = mid + 1;
      } else {
         hi = mid;
      }
   }
   first[entry] = lo;
}

// ------------------------------------------------------------------------------------------------
// The runs of the missing symbol.  k_missing_runs walks the plane [P][Wp] of the symbol along the positions: a wave owns one
// word column (64 consecutive sequences, one per lane), the 8 waves of a block the 8 columns of a 64-byte sector, so that the
// block reads every sector of the plane once.  WRITE = false counts the runs, WRITE = true emits them (sequence << 32 |
// start, end) through one atomic cursor; they are sorted afterwards.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t RUN_BLOCK_THREADS = 512;

template <bool WRITE>
__global__ __launch_bounds__(RUN_BLOCK_THREADS) void k_missing_runs(
   const uint64_t* __restrict__ plane, uint32_t positions, uint32_t row_words, unsigned long long* __restrict__ n_runs, uint64_t* __restrict__ run_keys,
   uint32_t* __restrict__ run_ends, unsigned long long capacity
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t word = blockIdx.x * (RUN_BLOCK_THREADS / 64) + (threadIdx.x >> 6);
   if (word >= row_words) {
      return;  // (uniform per wave)
   }
   const uint32_t sequence = word * 64u + lane;
   bool in_run = false;
   uint32_t start = 0;
   uint32_t counted = 0;
   const auto emit = [&](bool ends_here, uint32_t end) {
      if constexpr (WRITE) {
         const uint64_t ending = __ballot(ends_here);
         if (ending != 0) {
            unsigned long long first = 0;
            if (lane == static_cast<uint32_t>(__builtin_ctzll(ending))) {
               first = atomicAdd(n_runs, static_cast<unsigned long long>(__popcll(ending)));
            }
            first = __shfl(first, __builtin_ctzll(ending));
            const unsigned long long slot = first + static_cast<unsigned long long>(__popcll(ending & ((1ull << lane) - 1ull)));
            if (ends_here && slot < capacity) {
               run_keys[slot] = (static_cast<uint64_t>(sequence) << 32) | start;
               run_ends[slot] = end;
            }
         }
      } else {
         counted += ends_here ? 1u : 0u;
      }
   };
   constexpr uint32_t AHEAD = 8;  // plane words in flight per wave
   for (uint32_t base = 0; base < positions; base += AHEAD) {
      uint64_t words[AHEAD];
#pragma unroll
      for (uint32_t k = 0; k < AHEAD; ++k) {
         const uint32_t p = min(base + k, positions - 1u);
         words[k] = plane[static_cast<size_t>(p) * row_words + word];
      }
#pragma unroll
      for (uint32_t k = 0; k < AHEAD; ++k) {
         const uint32_t p = base + k;
         const bool inside = p < positions;  // (uniform) the last group may reach past the end: no state changes there
         const bool set = inside && ((words[k] >> lane) & 1ull) != 0;
         emit(inside && in_run && !set, p);
         if (set && !in_run) {
            start = p;
         }
         in_run = inside ? set : in_run;
      }
   }
   emit(in_run, positions);
   if constexpr (!WRITE) {
      const uint32_t wave_total = waveSumToLane63(counted);
      if (lane == 63u && wave_total != 0) {
         atomicAdd(n_runs, static_cast<unsigned long long>(wave_total));
      }
   }
}

// ------------------------------------------------------------------------------------------------
// The end runs of the gap symbol (SeqStoreHost::Layout::ends).  k_end_runs walks the build-time code planes
// [P][BITS][Wp] in the manner of k_missing_runs — a wave per word column, a lane per sequence — forward from position 0 and
// backward from P - 1, each walk stopping when no lane is still inside its run: lead[r] = the length of the maximal prefix of
// cells whose code is `code` (the gap symbol's), trail_start[r] = the first cell of the maximal suffix of them (P: none; a
// sequence that is the gap symbol throughout has lead = trail_start = P).  A run ends at the first cell that is anything else.
// ------------------------------------------------------------------------------------------------
template <int BITS>
__global__ __launch_bounds__(RUN_BLOCK_THREADS) void k_end_runs(
   const uint64_t* __restrict__ planes, uint32_t positions, uint32_t row_words, uint32_t sequence_count, uint32_t code, uint32_t* __restrict__ lead,
   uint32_t* __restrict__ trail_start
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t word = blockIdx.x * (RUN_BLOCK_THREADS / 64) + (threadIdx.x >> 6);
   if (word >= row_words) {
      return;  // (uniform per wave)
   }
   const uint32_t sequence = word * 64u + lane;
   const auto hasCode = [&](uint32_t p) {
      const uint64_t* base = planes + static_cast<size_t>(p) * BITS * row_words + word;
      bool match = true;
#pragma unroll
      for (int bit = 0; bit < BITS; ++bit) {
         match = match && ((base[static_cast<size_t>(bit) * row_words] >> lane) & 1ull) == ((code >> bit) & 1u);
      }
      return match;
   };
   bool inside = sequence < sequence_count;
   uint32_t n_lead = 0;
   for (uint32_t p = 0; p < positions && __ballot(inside) != 0; ++p) {
      inside = inside && hasCode(p);
      n_lead += inside ? 1u : 0u;
   }
   inside = sequence < sequence_count && n_lead < positions;
   uint32_t n_trail = 0;
   for (uint32_t p = positions; p-- > 0 && __ballot(inside) != 0;) {
      inside = inside && hasCode(p);
      n_trail += inside ? 1u : 0u;
   }
   if (sequence < sequence_count) {
      lead[sequence] = n_lead;
      trail_start[sequence] = positions - n_trail;
   }
}

/// hist[lead[r]] += 1 and hist[P + 1 + trail_start[r]] += 1 for every sequence (both arrays [P + 1]).
__global__ void k_end_histogram(const uint32_t* __restrict__ lead, const uint32_t* __restrict__ trail_start, uint32_t sequence_count, uint32_t positions, uint32_t* __restrict__ hist) {
   const uint32_t sequence = blockIdx.x * blockDim.x + threadIdx.x;
   if (sequence < sequence_count) {
      atomicAdd(&hist[lead[sequence]], 1u);
      atomicAdd(&hist[positions + 1u + trail_start[sequence]], 1u);
   }
}

/// The two end events of every sequence as 8-byte keys: kind 0 at lead, kind 1 at trail_start (those at P are left out later).
__global__ void k_end_events(const uint32_t* __restrict__ lead, const uint32_t* __restrict__ trail_start, uint32_t sequence_count, uint64_t* __restrict__ events) {
   const uint32_t sequence = blockIdx.x * blockDim.x + threadIdx.x;
   if (sequence < sequence_count) {
      events[2u * static_cast<size_t>(sequence)] = (static_cast<uint64_t>(lead[sequence]) << 37) | sequence;
      events[2u * static_cast<size_t>(sequence) + 1u] = (static_cast<uint64_t>(trail_start[sequence]) << 37) | (uint64_t{1} << 32) | sequence;
   }
}

/// The residual keys of the covered rows: a wave per word column, a lane per sequence, along the list of covered rows
/// (`rows`: their plane rows, `row_positions`: their positions) — a set bit outside the sequence's end runs gives the key
/// position << 37 | symbol << 32 | sequence, through one atomic cursor.
__global__ __launch_bounds__(RUN_BLOCK_THREADS) void k_residual_keys(
   const uint64_t* __restrict__ planes, uint32_t row_words, uint32_t sequence_count, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ row_positions,
   uint32_t n_rows, uint32_t symbol, const uint32_t* __restrict__ lead, const uint32_t* __restrict__ trail_start, unsigned long long* __restrict__ cursor,
   uint64_t* __restrict__ keys, unsigned long long capacity
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t word = blockIdx.x * (RUN_BLOCK_THREADS / 64) + (threadIdx.x >> 6);
   if (word >= row_words) {
      return;  // (uniform per wave)
   }
   const uint32_t sequence = word * 64u + lane;
   const bool real = sequence < sequence_count;
   const uint32_t own_lead = real ? lead[sequence] : 0u;
   const uint32_t own_trail = real ? trail_start[sequence] : 0u;
   for (uint32_t k = 0; k < n_rows; ++k) {
      const uint64_t bits = planes[static_cast<size_t>(rows[k]) * row_words + word];
      if (bits == 0) {
         continue;  // (uniform)
      }
      const uint32_t position = row_positions[k];
      const bool residual = real && ((bits >> lane) & 1ull) != 0 && own_lead <= position && position < own_trail;
      const uint64_t emitting = __ballot(residual);
      if (emitting != 0) {
         unsigned long long first = 0;
         if (lane == static_cast<uint32_t>(__builtin_ctzll(emitting))) {
            first = atomicAdd(cursor, static_cast<unsigned long long>(__popcll(emitting)));
         }
         first = __shfl(first, __builtin_ctzll(emitting));
         const unsigned long long slot = first + static_cast<unsigned long long>(__popcll(emitting & ((1ull << lane) - 1ull)));
         if (residual && slot < capacity) {
            keys[slot] = (static_cast<uint64_t>(position) << 37) | (static_cast<uint64_t>(symbol) << 32) | sequence;
         }
      }
   }
}

/// first[slice] = first run of the missing symbol whose sequence lies in slice `slice` of 2^ESCAPE_SLICE_SHIFT sequences or
/// beyond (the runs are sorted by sequence): one binary search per entry.
__global__ void k_run_slice_index(const uint64_t* __restrict__ run_keys, uint32_t n_runs, uint32_t slice_shift, uint32_t n_entries, uint32_t* __restrict__ first) {
   const uint32_t slice = blockIdx.x * blockDim.x + threadIdx.x;
   if (slice >= n_entries) {
      return;
   }
   uint32_t lo = 0, hi = n_runs;
   while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((static_cast<uint32_t>(run_keys[mid] >> 32) >> slice_shift) < slice) {
         lo = mid + 1;
      } else {
         hi = mid;
      }
   }
   first[slice] = lo;
}

/// The gap events of a store with derived symbols (SeqStoreHost::Layout::gaps): two per run of the missing symbol,
/// two per sparse key.  An empty run gives two events past the last position (left out by the slice index).
__global__ void k_gap_events(
   const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ run_ends, uint32_t n_runs, const uint64_t* __restrict__ sparse, uint32_t n_sparse,
   uint32_t positions, uint64_t* __restrict__ events
) {
   const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
   uint64_t sequence = 0, start = 0, end = 0;
   if (i < n_runs) {
      sequence = run_keys[i] >> 32;
      start = static_cast<uint32_t>(run_keys[i]);
      end = run_ends[i];
   } else if (i < n_runs + n_sparse) {
      sequence = static_cast<uint32_t>(sparse[i - n_runs]);
      start = sparse[i - n_runs] >> 37;
      end = start + 1u;
   } else {
      return;
   }
   if (start >= end) {
      start = end = positions;
   }
   events[2u * static_cast<size_t>(i)] = (start << 37) | sequence;
   events[2u * static_cast<size_t>(i) + 1u] = (end << 37) | (uint64_t{1} << 32) | sequence;
}

/// +1 where a run of the missing symbol starts, -1 where it ends: summed along the positions, the rows with the missing symbol.
__global__ void k_runs_diff_all(const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ run_ends, uint32_t n_runs, uint32_t* __restrict__ diff) {
   const uint32_t run = blockIdx.x * blockDim.x + threadIdx.x;
   if (run < n_runs) {
      atomicAdd(&diff[static_cast<uint32_t>(run_keys[run])], 1u);
      atomicAdd(&diff[run_ends[run]], 0xFFFFFFFFu);
   }
}

/// The two bounds of a granule of slice-major escape keys (SeqStoreHost::Layout::d_granule_heaviest, d_granule_without): the
/// largest weight[counter] and the largest without[position] over its keys; one block per granule.  A key that went to the
/// overflow list is no part of the stream and of its bounds.
__global__ __launch_bounds__(256) void k_granule_bounds(
   const uint32_t* __restrict__ packed, const uint32_t* __restrict__ granule_base, const uint32_t* __restrict__ weight, const uint32_t* __restrict__ without,
   uint32_t n_scan, uint32_t n_counters, uint32_t* __restrict__ heaviest_out, uint32_t* __restrict__ without_out
) {
   __shared__ uint32_t s_bounds[2];
   if (threadIdx.x < 2) {
      s_bounds[threadIdx.x] = 0;
   }
   __syncthreads();
   const uint32_t granule = blockIdx.x;
   const uint32_t base = granule_base[granule];
   uint32_t heaviest = 0, rows_without = 0;
   for (uint32_t k = threadIdx.x; k < ESCAPE_GRANULE_KEYS; k += blockDim.x) {
      const uint32_t key = packed[static_cast<size_t>(granule) * ESCAPE_GRANULE_KEYS + k];
      if (key != ESCAPE_KEY_INVALID) {
         const uint32_t counter = base + (key >> ESCAPE_SLICE_SHIFT);
         heaviest = max(heaviest, counter < n_counters ? weight[counter] : 0xFFFFFFFFu);
         rows_without = max(rows_without, counter < n_counters ? without[counter / n_scan] : 0xFFFFFFFFu);
      }
   }
   atomicMax(&s_bounds[0], heaviest);
   atomicMax(&s_bounds[1], rows_without);
   __syncthreads();
   if (threadIdx.x == 0) {
      heaviest_out[granule] = s_bounds[0];
      without_out[granule] = s_bounds[1];
   }
}

/// Does position p derive the reference's symbol?  What falls onto that symbol is never reported, so the keys and rows of the
/// position's other symbols may be left out where they are few (buildPruneBounds, buildRowBounds); every other position stays exact.
bool derivesReference(const SeqStoreHost& seqstore, uint32_t p) {
   const SeqStoreDev& dev = seqstore.dev;
   const uint8_t* map = seqstore.layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
   const uint8_t reference = seqstore.reference[p];
   return (map[0] & LAYOUT_IMPLICIT) != 0 && reference < dev.n_symbols && dev.kind[reference] == PLANE_SCAN && dev.index[reference] == map[IMPLICIT_SLOT];
}

/// The scan symbol of the gap symbol ('-', symbol 0 of both alphabets), or 0xFF where it is no scan symbol of the store.
uint32_t gapScanSymbol(const SeqStoreDev& dev) {
   return dev.n_symbols != 0 && dev.kind[0] == PLANE_SCAN ? dev.index[0] : 0xFFu;
}

}  // namespace

namespace silo_gpu_detail {

/// finalize(): the plane of the missing symbol becomes the list of its runs (PLANE_RUNS) where that takes less than a quarter
/// of the plane — always, for data whose missing cells come in runs — and the plane is released.
int compactMissingPlane(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreDev& dev = seqstore.dev;
   if (dev.runs_at_build != 0) {  // a two-pass build wrote the runs while the rows streamed in: they only have to be put in order
      dev.runs_at_build = 0;
      unsigned long long written = 0;
      HIP_TRY(hipMemcpy(&written, seqstore.d_run_count.get(), sizeof(written), hipMemcpyDeviceToHost));
      if (written != dev.enc_run_capacity) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "two-pass build: the second pass did not bring the rows the first pass counted (runs of the missing symbol differ)");
      }
      if (const int rc = silo_gpu_internal_sort_pairs(seqstore.d_missing_run_keys.get(), seqstore.d_missing_run_ends.get(), written); rc != SILO_GPU_OK) {
         return rc;
      }
      store->device_bytes += std::max<size_t>(written, 1) * (sizeof(uint64_t) + sizeof(uint32_t));
      dev.missing_run_keys = seqstore.d_missing_run_keys.get();
      dev.missing_run_ends = seqstore.d_missing_run_ends.get();
      dev.n_missing_runs = static_cast<uint32_t>(written);
      dev.kind[dev.missing_symbol] = PLANE_RUNS;
      return SILO_GPU_OK;
   }
   if (dev.n_extra != 1 || dev.extra == nullptr || dev.kind[dev.missing_symbol] != PLANE_EXTRA || dev.positions == 0 || missingRunsOption(store) < 0) {
      return SILO_GPU_OK;
   }
   const size_t plane_bytes = static_cast<size_t>(dev.positions) * dev.row_words * sizeof(uint64_t);
   DeviceArray<unsigned long long> d_count;
   HIP_TRY(d_count.alloc(1));
   const auto count_runs = [&](bool write, uint64_t* keys, uint32_t* ends, unsigned long long capacity, unsigned long long* out) -> int {
      HIP_TRY(hipMemset(d_count.get(), 0, sizeof(unsigned long long)));
      const uint32_t blocks = (dev.row_words + RUN_BLOCK_THREADS / 64 - 1) / (RUN_BLOCK_THREADS / 64);
      const auto walk = write ? k_missing_runs<true> : k_missing_runs<false>;
      walk<<<blocks, RUN_BLOCK_THREADS>>>(dev.extra, dev.positions, dev.row_words, d_count.get(), keys, ends, capacity);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(out, d_count.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
      return SILO_GPU_OK;
   };
   unsigned long long n_runs = 0;
   if (const int rc = count_runs(false, nullptr, nullptr, 0, &n_runs);
       rc != SILO_GPU_OK || n_runs >= (1ull << 32) || n_runs * (sizeof(uint64_t) + sizeof(uint32_t)) > plane_bytes / 4) {
      return rc;  // scattered missing cells: the plane stays
   }
   DeviceArray<uint64_t> d_keys;
   DeviceArray<uint32_t> d_ends;
   const size_t slots = std::max<size_t>(n_runs, 1);
   HIP_TRY(d_keys.alloc(slots));
   HIP_TRY(d_ends.alloc(slots));
   unsigned long long written = 0;
   if (const int rc = count_runs(true, d_keys.get(), d_ends.get(), n_runs, &written); rc != SILO_GPU_OK) {
      return rc;
   }
   if (written != n_runs) {
      return fail(SILO_GPU_ERR_HIP, "runs of the missing symbol: the two passes over the plane disagree");
   }
   if (const int rc = silo_gpu_internal_sort_pairs(d_keys.get(), d_ends.get(), n_runs); rc != SILO_GPU_OK) {  // by (sequence, start)
      return rc;
   }
   d_count.reset();
   seqstore.d_extra.reset();  // before the adaptive planes are allocated: a lower peak
   dev.extra = nullptr;
   store->device_bytes -= plane_bytes;
   store->device_bytes += slots * (sizeof(uint64_t) + sizeof(uint32_t));
   seqstore.d_missing_run_keys = std::move(d_keys);
   seqstore.d_missing_run_ends = std::move(d_ends);
   dev.missing_run_keys = seqstore.d_missing_run_keys.get();
   dev.missing_run_ends = seqstore.d_missing_run_ends.get();
   dev.n_missing_runs = static_cast<uint32_t>(n_runs);
   dev.kind[dev.missing_symbol] = PLANE_RUNS;
   return SILO_GPU_OK;
}

/// A store with derived symbols counts, per scan, the rows of the filter inside a run of the missing symbol: where the runs
/// of every slice of sequences begin (k_scan_missing_runs keeps that slice of the filter in LDS).
int buildRunSliceIndex(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreHost::Layout& layout = seqstore.layout;
   if (!layout.has_implicit || layout.d_run_slice_first.get() != nullptr) {
      return SILO_GPU_OK;
   }
   const SeqStoreDev& dev = seqstore.dev;
   if (dev.kind[dev.missing_symbol] != PLANE_RUNS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "a store with derived symbols keeps the missing symbol as runs");
   }
   layout.n_run_slices = sliceCount(store->sequence_count);
   const uint32_t n_entries = layout.n_run_slices + 1;
   HIP_TRY(layout.d_run_slice_first.alloc(n_entries));
   k_run_slice_index<<<(n_entries + 255) / 256, 256>>>(dev.missing_run_keys, dev.n_missing_runs, ESCAPE_SLICE_SHIFT, n_entries, layout.d_run_slice_first.get());
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipStreamSynchronize(nullptr));
   return SILO_GPU_OK;
}

/// `d_sorted` — n_keys keys in ascending order, the caller's scratch — is sorted slice-major (stably: (position, symbol,
/// sequence) order within a slice), indexed [slice][position] and packed into `out` (left as it was where this fails);
/// counter = position * n_scan + symbol.
/// max_span = 0: every slice's keys are cut into whole granules, and a key whose counter lies more than ESCAPE_MAX_RELATIVE past
/// its granule's first goes to the overflow list.  max_span > 0: a granule also ends early where its next key's position lies
/// more than max_span positions past its first key's (the rest is padding), so that no key overflows.  Keys at or past
/// `positions` are left out.
int packSliceMajor(uint64_t* d_sorted, uint64_t n_keys, uint32_t n_scan, uint32_t positions, uint32_t n_slices, uint32_t max_span, SliceMajorKeys& out) {
   const size_t n_entries = static_cast<size_t>(n_slices) * (positions + 1);
   SliceMajorKeys packed;
   DeviceArray<uint32_t> d_unpacked, d_overflow_count;
   const char* const what = "slice-major keys";
   if (const int rc = silo_gpu_internal_sort_keys_by_bits(d_sorted, n_keys, ESCAPE_SLICE_SHIFT, ESCAPE_SLICE_SHIFT + ESCAPE_SLICE_BITS); rc != SILO_GPU_OK) {
      return rc;
   }
   hipError_t status = packed.d_slice_first.alloc(n_entries);
   if (status != hipSuccess) {
      return failHip(what, status);
   }
   k_slice_index<<<static_cast<uint32_t>((n_entries + 255) / 256), 256>>>(d_sorted, static_cast<uint32_t>(n_keys), ESCAPE_SLICE_SHIFT, n_slices, positions, packed.d_slice_first.get());
   packed.slice_first.resize(n_entries);
   status = hipGetLastError();
   status = status != hipSuccess ? status : hipMemcpy(packed.slice_first.data(), packed.d_slice_first.get(), n_entries * sizeof(uint32_t), hipMemcpyDeviceToHost);
   if (status != hipSuccess) {
      return failHip(what, status);
   }
   // every slice's keys cut into granules (padded to whole ones); the index [slice][position] moves to the packed numbering
   std::vector<uint32_t> unpacked_first, unpacked_end;
   for (uint32_t slice = 0; slice < n_slices; ++slice) {
      uint32_t* first = packed.slice_first.data() + static_cast<size_t>(slice) * (positions + 1);
      const uint32_t slice_begin = first[0];
      const uint32_t slice_end = first[positions];
      const size_t slice_granule = unpacked_first.size();
      for (uint32_t at = slice_begin; at < slice_end;) {
         uint32_t end = std::min(slice_end, at + ESCAPE_GRANULE_KEYS);
         if (max_span != 0) {  // the position of the key `at`, and the keys within max_span positions of it
            const uint32_t position = static_cast<uint32_t>(std::upper_bound(first, first + positions + 1, at) - first) - 1u;
            end = std::min(end, first[std::min<uint64_t>(positions, static_cast<uint64_t>(position) + max_span + 1u)]);
         }
         unpacked_first.push_back(at);
         unpacked_end.push_back(end);
         at = end;
      }
      size_t g = slice_granule;
      for (uint32_t p = 0; p <= positions; ++p) {
         const uint32_t at = first[p];
         while (g + 1 < unpacked_first.size() && unpacked_first[g + 1] <= at) {
            ++g;
         }
         first[p] = g < unpacked_first.size() ? static_cast<uint32_t>(g * ESCAPE_GRANULE_KEYS + (at - unpacked_first[g])) : static_cast<uint32_t>(g * ESCAPE_GRANULE_KEYS);
      }
   }
   const size_t n_granules = unpacked_first.size();
   packed.packed_keys = static_cast<uint64_t>(n_granules) * ESCAPE_GRANULE_KEYS;
   const uint32_t overflow_capacity = max_span != 0 ? 0u : static_cast<uint32_t>(std::min<uint64_t>(n_keys, uint64_t{1} << 26));
   if (packed.packed_keys >= (uint64_t{1} << 32)) {
      return fail(SILO_GPU_ERR_UNSUPPORTED, "more than 2^32 packed escape keys in one sequence store");
   }
   status = packed.d_keys.alloc(packed.packed_keys + 4);  // (16-byte loads: a quad of slack)
   status = status != hipSuccess ? status : packed.d_granule_base.alloc(std::max<size_t>(n_granules, 1));
   status = status != hipSuccess ? status : d_unpacked.alloc(std::max<size_t>(n_granules, 1) * 2);
   status = status != hipSuccess ? status : d_overflow_count.alloc(1);
   status = status != hipSuccess ? status : packed.d_overflow.alloc(std::max<size_t>(overflow_capacity, 1));
   status = status != hipSuccess ? status : hipMemset(d_overflow_count.get(), 0, sizeof(uint32_t));
   status = status != hipSuccess ? status : hipMemcpy(d_unpacked.get(), unpacked_first.data(), n_granules * sizeof(uint32_t), hipMemcpyHostToDevice);
   status = status != hipSuccess ? status : hipMemcpy(d_unpacked.get() + n_granules, unpacked_end.data(), n_granules * sizeof(uint32_t), hipMemcpyHostToDevice);
   status = status != hipSuccess ? status : hipMemcpy(packed.d_slice_first.get(), packed.slice_first.data(), n_entries * sizeof(uint32_t), hipMemcpyHostToDevice);
   if (status == hipSuccess && n_granules > 0) {
      k_pack_sliced_keys<<<static_cast<uint32_t>(n_granules), 256>>>(
         d_sorted, d_unpacked.get(), d_unpacked.get() + n_granules, n_scan, packed.d_keys.get(), packed.d_granule_base.get(), packed.d_overflow.get(),
         d_overflow_count.get(), overflow_capacity
      );
      status = hipGetLastError();
   }
   status = status != hipSuccess ? status : hipMemcpy(&packed.n_overflow, d_overflow_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost);
   if (status != hipSuccess) {
      return failHip(what, status);
   }
   if (packed.n_overflow > overflow_capacity) {
      return fail(SILO_GPU_ERR_UNSUPPORTED, "too many escape keys outside their granule's counter range");
   }
   if (packed.n_overflow == 0) {
      packed.d_overflow.reset();
   }
   packed.n_slices = n_slices;
   out = std::move(packed);
   return SILO_GPU_OK;
}

/// The gap events of a store with derived symbols, slice-major and packed: the scan's escape pass counts them with the keys.
int buildGapEvents(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreHost::Layout& layout = seqstore.layout;
   const SeqStoreDev& dev = seqstore.dev;
   const uint32_t n_slices = sliceCount(store->sequence_count);
   const uint64_t n_sparse = seqstore.sparse_sorted.size();
   const uint64_t n_events = 2u * (static_cast<uint64_t>(dev.n_missing_runs) + n_sparse);
   if (!layout.has_implicit || layout.gap_stream || n_slices > ESCAPE_MAX_SLICES || n_events >= (uint64_t{1} << 31)) {
      return SILO_GPU_OK;  // (too many events: the scan takes the runs and the sparse keys by themselves)
   }
   if (n_events != 0) {
      DeviceArray<uint64_t> d_events;
      HIP_TRY(d_events.alloc(n_events));
      const uint32_t n_intervals = static_cast<uint32_t>(n_events / 2u);
      k_gap_events<<<(n_intervals + 255) / 256, 256>>>(
         dev.missing_run_keys, dev.missing_run_ends, dev.n_missing_runs, seqstore.d_sparse.get(), static_cast<uint32_t>(n_sparse), dev.positions, d_events.get()
      );
      if (hipGetLastError() != hipSuccess) {
         return fail(SILO_GPU_ERR_HIP, "gap events: the launch failed");
      }
      if (const int rc = silo_gpu_internal_sort_keys(d_events.get(), n_events); rc != SILO_GPU_OK) {  // ascending: (position, kind, sequence)
         return rc;
      }
      if (const int rc = packSliceMajor(d_events.get(), n_events, 2, dev.positions, n_slices, GAP_MAX_SPAN, layout.gaps); rc != SILO_GPU_OK) {
         return rc;
      }
   }
   layout.gap_stream = true;
   // (not charged to device_bytes: the stream is a scan-side copy of the runs and sparse keys, as d_run_slice_first is, and
   // its padding depends on how the runs of a row were cut by the build)
   return SILO_GPU_OK;
}

/// without[p] = the rows of the store without a valid symbol at position p: those inside a run of the missing symbol plus the
/// sparsely stored symbols (ambiguity codes) there — what the gap events of the store count under the full filter.
int rowsWithoutSymbol(const SeqStoreHost& seqstore, std::vector<uint32_t>& without) {
   const SeqStoreDev& dev = seqstore.dev;
   const uint32_t positions = dev.positions;
   std::vector<uint32_t> diff(positions + 1, 0);
   if (dev.n_missing_runs != 0) {
      DeviceArray<uint32_t> d_diff;
      HIP_TRY(d_diff.alloc(diff.size()));
      HIP_TRY(hipMemset(d_diff.get(), 0, diff.size() * sizeof(uint32_t)));
      k_runs_diff_all<<<(dev.n_missing_runs + 255) / 256, 256>>>(dev.missing_run_keys, dev.missing_run_ends, dev.n_missing_runs, d_diff.get());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(diff.data(), d_diff.get(), diff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   }
   without.assign(positions, 0);
   uint32_t missing = 0;
   for (uint32_t p = 0; p < positions; ++p) {
      missing += diff[p];
      without[p] = missing;
   }
   for (const uint64_t key : seqstore.sparse_sorted) {
      const uint64_t position = key >> 37;
      if (position < positions) {
         without[position] += 1;
      }
   }
   return SILO_GPU_OK;
}

/// The bounds per granule of escape keys that let a Mutations scan leave out keys no reported row can come from
/// (silo_gpu_mutations_scan_ranges_min_proportion).  At a position whose derived symbol is the reference's, the keys of a
/// (position, symbol) group that is small against the filter only move their count onto a symbol that is never reported; what
/// "small" means needs the group's size in the whole store and the rows of the store without a valid symbol at the position.
/// Built only where the store has its gap events (the scan prunes on that path alone).
int buildPruneBounds(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreHost::Layout& layout = seqstore.layout;
   const SeqStoreDev& dev = seqstore.dev;
   const SliceMajorKeys& keys = layout.escapes_sliced;
   if (!layout.built || !layout.has_implicit || !layout.gap_stream || keys.d_keys.get() == nullptr || layout.d_granule_heaviest.get() != nullptr) {
      return SILO_GPU_OK;
   }
   const uint32_t positions = dev.positions;
   const size_t n_counters = static_cast<size_t>(positions) * dev.n_scan;
   const size_t n_granules = keys.packed_keys / ESCAPE_GRANULE_KEYS;
   if (n_granules == 0 || n_counters >= (uint64_t{1} << 32)) {
      return SILO_GPU_OK;
   }
   std::vector<uint32_t> without;
   if (const int rc = rowsWithoutSymbol(seqstore, without); rc != SILO_GPU_OK) {
      return rc;
   }
   // the keys of a (position, symbol) in the whole store; UINT32_MAX — never left out — where the position derives no symbol or
   // another one than the reference's (that symbol is reported, so its count has to be exact)
   std::vector<uint32_t> weight(n_counters);
   for (uint32_t p = 0; p < positions; ++p) {
      const bool prunable = derivesReference(seqstore, p);
      for (uint32_t symbol = 0; symbol < dev.n_scan; ++symbol) {
         const size_t counter = static_cast<size_t>(p) * dev.n_scan + symbol;
         weight[counter] = prunable ? layout.escape_first_symbol[counter + 1] - layout.escape_first_symbol[counter] : 0xFFFFFFFFu;
      }
   }
   DeviceArray<uint32_t> d_weight, d_without, d_granule_heaviest, d_granule_without;
   std::vector<uint32_t> granule_heaviest(n_granules, 0xFFFFFFFFu), granule_without(n_granules, 0xFFFFFFFFu);
   HIP_TRY(d_weight.alloc(n_counters));
   HIP_TRY(d_without.alloc(positions));
   HIP_TRY(d_granule_heaviest.alloc(n_granules));
   HIP_TRY(d_granule_without.alloc(n_granules));
   HIP_TRY(hipMemcpy(d_weight.get(), weight.data(), n_counters * sizeof(uint32_t), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(d_without.get(), without.data(), static_cast<size_t>(positions) * sizeof(uint32_t), hipMemcpyHostToDevice));
   k_granule_bounds<<<static_cast<uint32_t>(n_granules), 256>>>(
      keys.d_keys.get(), keys.d_granule_base.get(), d_weight.get(), d_without.get(), dev.n_scan, static_cast<uint32_t>(n_counters), d_granule_heaviest.get(),
      d_granule_without.get()
   );
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipMemcpy(granule_heaviest.data(), d_granule_heaviest.get(), n_granules * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(granule_without.data(), d_granule_without.get(), n_granules * sizeof(uint32_t), hipMemcpyDeviceToHost));
   layout.d_granule_heaviest = std::move(d_granule_heaviest);
   layout.d_granule_without = std::move(d_granule_without);
   layout.granule_heaviest = std::move(granule_heaviest);
   layout.granule_without = std::move(granule_without);
   const uint64_t bytes = 2u * n_granules * sizeof(uint32_t);
   layout.device_bytes += bytes;
   store->device_bytes += bytes;
   return SILO_GPU_OK;
}

/// The same two bounds per one-hot plane row (SeqStoreHost::Layout::d_row_heaviest, d_row_without), so that the scan may leave
/// out whole rows by the rule it leaves out granules of keys by.  A row holds every row of the store with its symbol at its
/// position: its weight is the store's total of that (position, symbol), and the rows without a valid symbol are those of its
/// own position.  Built where the store has its gap events and its totals; a store without either keeps null pointers.
int buildRowBounds(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreHost::Layout& layout = seqstore.layout;
   const SeqStoreDev& dev = seqstore.dev;
   if (!layout.built || !layout.has_implicit || !layout.gap_stream || layout.d_row_target.get() == nullptr || layout.d_row_heaviest.get() != nullptr ||
       seqstore.d_totals.get() == nullptr || !seqstore.totals_ready || layout.row_of.size() != static_cast<size_t>(dev.positions) + 1) {
      return SILO_GPU_OK;
   }
   const uint32_t positions = dev.positions;
   const size_t n_rows = layout.row_of[positions];
   bool any_one_hot = false;
   for (const SeqStoreHost::Run& run : layout.runs) {
      any_one_hot = any_one_hot || (run.one_hot && layout.row_of[run.end] != layout.row_of[run.begin]);
   }
   if (!any_one_hot) {
      return SILO_GPU_OK;
   }
   std::vector<uint32_t> without, totals;
   if (const int rc = rowsWithoutSymbol(seqstore, without); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = downloadTotals(seqstore, totals); rc != SILO_GPU_OK) {
      return rc;
   }
   std::vector<uint32_t> row_heaviest(n_rows, 0xFFFFFFFFu), row_without(n_rows, 0xFFFFFFFFu);
   for (uint32_t p = 0; p < positions; ++p) {
      const uint8_t* map = layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
      bool prunable = (map[0] & LAYOUT_ONE_HOT) != 0 && derivesReference(seqstore, p);
      if (prunable) {
         // ... and holds the majority of the position's valid rows.  The rows this is for are those of a settled position (a
         // lineage's substitution, the flank of a ragged end: a few percent beside one symbol); a position that several symbols
         // share keeps every cell exact, as a block of code planes does — the key pass keeps such cells as well, its granules
         // reaching across their neighbours.
         uint64_t valid = 0;
         for (uint32_t symbol = 0; symbol < dev.n_scan; ++symbol) {
            valid += totals[static_cast<size_t>(p) * dev.n_scan + symbol];
         }
         prunable = 2u * static_cast<uint64_t>(totals[static_cast<size_t>(p) * dev.n_scan + map[IMPLICIT_SLOT]]) > valid;
      }
      for (uint32_t row = layout.row_of[p]; prunable && row < layout.row_of[p + 1]; ++row) {
         const uint8_t symbol = map[1 + (row - layout.row_of[p])];
         if (symbol < dev.n_scan) {  // (a row without a symbol is empty and stays as it is)
            row_heaviest[row] = totals[static_cast<size_t>(p) * dev.n_scan + symbol];
            row_without[row] = without[p];
         }
      }
   }
   DeviceArray<uint32_t> d_row_heaviest, d_row_without;
   HIP_TRY(d_row_heaviest.alloc(n_rows));
   HIP_TRY(d_row_without.alloc(n_rows));
   HIP_TRY(hipMemcpy(d_row_heaviest.get(), row_heaviest.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(d_row_without.get(), row_without.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
   layout.d_row_heaviest = std::move(d_row_heaviest);
   layout.d_row_without = std::move(d_row_without);
   layout.row_heaviest = std::move(row_heaviest);
   layout.row_without = std::move(row_without);
   const uint64_t bytes = 2u * n_rows * sizeof(uint32_t);
   layout.device_bytes += bytes;
   store->device_bytes += bytes;
   return SILO_GPU_OK;
}

/// finalize(), while the build-time planes are still there: where every sequence's leading run of the gap symbol ends and its
/// trailing run begins (k_end_runs), for buildEndRuns.  Only for a store that derives symbols — no other store gets gap events.
int walkEndRuns(silo_gpu_store* store, SeqStoreHost& seqstore, bool has_implicit) {
   const SeqStoreDev& dev = seqstore.dev;
   SeqStoreHost::Layout& layout = seqstore.layout;
   const uint32_t symbol = gapScanSymbol(dev);
   if (!has_implicit || dev.scan == nullptr || symbol == 0xFFu || sliceCount(store->sequence_count) > ESCAPE_MAX_SLICES || dev.positions == 0 ||
       layout.d_end_lead.get() != nullptr || (dev.n_bits != 3 && dev.n_bits != 5)) {
      return SILO_GPU_OK;
   }
   DeviceArray<uint32_t> d_lead, d_trail;
   HIP_TRY(d_lead.alloc(store->sequence_count));
   HIP_TRY(d_trail.alloc(store->sequence_count));
   const uint32_t blocks = (dev.row_words + RUN_BLOCK_THREADS / 64 - 1) / (RUN_BLOCK_THREADS / 64);
   const auto walk = dev.n_bits == 3 ? k_end_runs<3> : k_end_runs<5>;
   walk<<<blocks, RUN_BLOCK_THREADS>>>(dev.scan, dev.positions, dev.row_words, store->sequence_count, symbol + 1u, d_lead.get(), d_trail.get());
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipStreamSynchronize(nullptr));  // the planes are released next
   layout.d_end_lead = std::move(d_lead);
   layout.d_end_trail = std::move(d_trail);
   return SILO_GPU_OK;
}

/// The end runs of the gap symbol for the Mutations scan (SeqStoreHost::Layout::ends and what goes with it): which
/// one-hot rows of the gap symbol the scan may count from the sequences' ends instead (endRunCovers), the end events, and the
/// residual keys of the covered rows.  Built where the store has its gap events and finalize walked the build-time planes
/// (walkEndRuns); every other store — two-pass builds, imports, more than ESCAPE_MAX_SLICES slices, nothing derived — has none
/// and is scanned row by row.  Nothing of the store itself changes.
int buildEndRuns(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreHost::Layout& layout = seqstore.layout;
   const SeqStoreDev& dev = seqstore.dev;
   // what walkEndRuns left for this stage goes when it returns, whichever way
   const DeviceArray<uint32_t> d_lead = std::move(layout.d_end_lead), d_trail = std::move(layout.d_end_trail);
   DeviceArray<uint32_t> d_hist;
   DeviceArray<uint32_t> d_rows;  // the covered rows, then their positions
   DeviceArray<uint64_t> d_keys;
   DeviceArray<unsigned long long> d_cursor;
   const uint32_t positions = dev.positions;
   const uint32_t sequences = store->sequence_count;
   const uint32_t symbol = gapScanSymbol(dev);
   if (d_lead.get() == nullptr || !layout.built || !layout.has_implicit || !layout.gap_stream || layout.d_row_target.get() == nullptr || layout.planes.get() == nullptr ||
       seqstore.d_totals.get() == nullptr || !seqstore.totals_ready || layout.row_of.size() != static_cast<size_t>(positions) + 1 || layout.ends.d_keys.get() != nullptr) {
      return SILO_GPU_OK;
   }
   const uint32_t n_slices = sliceCount(sequences);
   // how many leading runs end, and trailing runs begin, at every position
   std::vector<uint32_t> hist(2 * (static_cast<size_t>(positions) + 1));
   HIP_TRY(d_hist.alloc(hist.size()));
   HIP_TRY(hipMemset(d_hist.get(), 0, hist.size() * sizeof(uint32_t)));
   k_end_histogram<<<(sequences + 255) / 256, 256>>>(d_lead.get(), d_trail.get(), sequences, positions, d_hist.get());
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipMemcpy(hist.data(), d_hist.get(), hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   std::vector<uint32_t> totals;
   if (const int rc = downloadTotals(seqstore, totals); rc != SILO_GPU_OK) {
      return rc;
   }
   // the covered rows
   const uint64_t row_bytes = static_cast<uint64_t>(dev.row_words) * sizeof(uint64_t);
   const uint64_t key_cost = keyCostOption(store) > 0 ? static_cast<uint64_t>(keyCostOption(store)) : KEY_COST_BYTES;
   const size_t n_rows = layout.row_of[positions];
   std::vector<uint8_t> row_covered(n_rows, 0), position_covered(positions, 0);
   std::vector<uint32_t> covered_list, covered_positions;
   uint64_t ends_before = 0, trails_from = 0, residual_total = 0, events = 0;
   for (uint32_t p = 0; p < positions; ++p) {
      ends_before += hist[p];
      trails_from += hist[static_cast<size_t>(positions) + 1 + p];
      events += hist[p] + hist[static_cast<size_t>(positions) + 1 + p];
      const uint8_t* map = layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
      for (uint32_t row = layout.row_of[p]; (map[0] & LAYOUT_ONE_HOT) != 0 && row < layout.row_of[p + 1]; ++row) {
         if (map[1 + (row - layout.row_of[p])] != symbol) {
            continue;
         }
         const uint64_t residual = silo_gpu_layout::endRunResidual(totals[static_cast<size_t>(p) * dev.n_scan + symbol], sequences, ends_before, trails_from);
         if (silo_gpu_layout::endRunCovers(map[0], map[IMPLICIT_SLOT], symbol, residual, row_bytes, key_cost)) {
            row_covered[row] = 1;
            position_covered[p] = 1;
            covered_list.push_back(row);
            covered_positions.push_back(p);
            residual_total += residual;
         }
      }
   }
   if (!silo_gpu_layout::endRunsPay(covered_list.size(), row_bytes, events, residual_total, key_cost) || 2u * static_cast<uint64_t>(sequences) >= (uint64_t{1} << 31) ||
       residual_total >= (uint64_t{1} << 31)) {
      return SILO_GPU_OK;  // nothing to gain (a few covered rows against an event per sequence end): the scan reads every row
   }
   // the residual keys: the bits of the covered rows outside every end run
   SliceMajorKeys residual;
   if (residual_total != 0) {
      const size_t n_covered = covered_list.size();
      unsigned long long written = 0;
      HIP_TRY(d_rows.alloc(2 * n_covered));
      HIP_TRY(d_keys.alloc(residual_total));
      HIP_TRY(d_cursor.alloc(1));
      HIP_TRY(hipMemset(d_cursor.get(), 0, sizeof(unsigned long long)));
      HIP_TRY(hipMemcpy(d_rows.get(), covered_list.data(), n_covered * sizeof(uint32_t), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d_rows.get() + n_covered, covered_positions.data(), n_covered * sizeof(uint32_t), hipMemcpyHostToDevice));
      const uint32_t blocks = (dev.row_words + RUN_BLOCK_THREADS / 64 - 1) / (RUN_BLOCK_THREADS / 64);
      k_residual_keys<<<blocks, RUN_BLOCK_THREADS>>>(
         layout.planes.get(), dev.row_words, sequences, d_rows.get(), d_rows.get() + n_covered, static_cast<uint32_t>(n_covered), symbol, d_lead.get(),
         d_trail.get(), d_cursor.get(), d_keys.get(), residual_total
      );
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(&written, d_cursor.get(), sizeof(written), hipMemcpyDeviceToHost));
      if (written != residual_total) {
         return fail(SILO_GPU_ERR_HIP, "end runs: the covered rows hold other bits outside the end runs than their totals say");
      }
      if (const int rc = silo_gpu_internal_sort_keys(d_keys.get(), residual_total); rc != SILO_GPU_OK) {  // ascending: (position, symbol, sequence)
         return rc;
      }
      // (granules that end early instead of an overflow list, as the gap events have them: the keys lie hundreds to a position
      // at the two ends of the alignment and nowhere between, and an overflow list would be a launch of its own in every scan)
      const uint32_t max_span = (ESCAPE_MAX_RELATIVE + 1u - dev.n_scan) / dev.n_scan;
      if (const int rc = packSliceMajor(d_keys.get(), residual_total, dev.n_scan, positions, n_slices, max_span, residual); rc != SILO_GPU_OK) {
         return rc;
      }
      d_keys.reset();  // before the end events are allocated
   }
   // the end events
   const uint64_t n_events = 2u * static_cast<uint64_t>(sequences);
   SliceMajorKeys ends;
   hipError_t status = d_keys.alloc(n_events);
   if (status == hipSuccess) {
      k_end_events<<<(sequences + 255) / 256, 256>>>(d_lead.get(), d_trail.get(), sequences, d_keys.get());
      status = hipGetLastError();
   }
   if (status != hipSuccess) {
      return failHip("end events", status);
   }
   if (const int rc = silo_gpu_internal_sort_keys(d_keys.get(), n_events); rc != SILO_GPU_OK) {  // ascending: (position, kind, sequence)
      return rc;
   }
   if (const int rc = packSliceMajor(d_keys.get(), n_events, 2, positions, n_slices, GAP_MAX_SPAN, ends); rc != SILO_GPU_OK) {
      return rc;
   }
   DeviceArray<uint8_t> d_row_covered, d_position_covered;
   status = d_row_covered.alloc(std::max<size_t>(n_rows, 1));
   status = status != hipSuccess ? status : d_position_covered.alloc(positions);
   status = status != hipSuccess ? status : hipMemcpy(d_row_covered.get(), row_covered.data(), n_rows, hipMemcpyHostToDevice);
   status = status != hipSuccess ? status : hipMemcpy(d_position_covered.get(), position_covered.data(), positions, hipMemcpyHostToDevice);
   if (status != hipSuccess) {
      return failHip("end runs", status);
   }
   layout.ends = std::move(ends);
   layout.end_events = events;
   layout.residual = std::move(residual);
   layout.residual_keys = residual_total;
   layout.d_row_covered = std::move(d_row_covered);
   layout.d_position_covered = std::move(d_position_covered);
   layout.row_covered = std::move(row_covered);
   layout.position_covered = std::move(position_covered);
   layout.covered_rows = covered_list.size();
   layout.end_symbol = symbol;
   // (not charged to device_bytes, as the gap events are not: scan-side copies of what the rows hold)
   return SILO_GPU_OK;
}

}  // namespace silo_gpu_detail
