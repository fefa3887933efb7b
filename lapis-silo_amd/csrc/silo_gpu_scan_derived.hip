// silo_gpu_scan_derived.hip — the passes of K1, the Mutations scan, for derived symbols (LAYOUT_IMPLICIT; DESIGN.md §3, "The
// passes for derived symbols"): the count of a position's most numerous symbol is what is left of the filter.
//
// Kernels:
//   k_scan_missing_runs<LDS_DIFF>, k_sum_run_parts   rows of the filter inside a run of the missing symbol, per position
//   k_count_sparse_keys                              rows of the filter with an ambiguity code, per position
//   k_finish_scan<EVENTS, SELECT>                    derived counts; the scan's private tables into the caller's — or over them, with K4's row selection
// (k_scan_missing_runs and k_count_sparse_keys run only where a store has no gap events: SILO_GPU_TUNE_GAP_EVENTS < 0.)
// Exported (scan_internal.h): planDerived, bindDerived, scanRowsWithoutSymbol, finishDerived.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <array>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "fused_select_rule.h"
#include "scan_internal.h"

using namespace silo_gpu_detail;

namespace {

// ------------------------------------------------------------------------------------------------
// Derived symbols (LAYOUT_IMPLICIT).  At almost every position of an alignment ONE symbol has nearly every row.  The reference
// leaves that symbol's bitmap out and rebuilds its count as |filter| - #missing - the other symbols' counts
// (position.cpp:102-127, mutations.cpp:74-95); the dense restatement of the same idea: such a position stores NO row for that
// symbol, and a scan
//   1. counts the other valid symbols as ever (their one-hot rows, their escape keys) — into PRIVATE tables in scratch,
//   2. counts, per position, the rows of the filter that have no valid symbol there: those inside a run of the missing symbol
//      (k_scan_missing_runs: +1 where a selected row's run starts, -1 where it ends, summed along the positions afterwards)
//      and those with an ambiguity code (k_count_sparse_keys),
//   3. k_finish_scan: derived count = |filter| - (2.) - sum of (1.) at the position; private tables -> the caller's.
// Where the store has its gap events (SeqStoreHost::Layout::gaps), 2. is part of the escape pass instead: the events
// are one more range of k_scan_escapes_sliced, counted into gaps[n][2], and k_finish_scan<true> sums starts less ends.
// The filter's cardinality comes from the prepare step (k_compact_filter, counter [2]).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t DERIVED_THREADS = 1024;
constexpr uint32_t SPARSE_KEYS_PER_THREAD = 4;
constexpr uint32_t RUNS_IN_FLIGHT = 4;        // runs per thread whose loads are in flight together (k_scan_missing_runs)


/// grid = (blocks per slice, slice of 2^17 sequences x range, filter).  The block keeps its slice of the filter in LDS (16 KiB) and, where it
/// fits (LDS_DIFF), the diff of the whole range as well (<= ~140 KiB: 35 000 positions), so that the adds of a slice's runs —
/// two per selected run — are LDS atomics and only the non-zero entries go to memory (256 contiguous bytes per wave instruction).
template <bool LDS_DIFF>
__global__ __launch_bounds__(DERIVED_THREADS) void k_scan_missing_runs(const DerivedArgs args) {
   extern __shared__ uint32_t s_runs[];  // [ESCAPE_SLICE_WORDS32] the filter slice, then [n + 1] the diff
   uint32_t* s_diff = s_runs + ESCAPE_SLICE_WORDS32;
   const uint32_t q = blockIdx.z;
   const uint32_t slice = blockIdx.y % args.n_run_slices;
   const DerivedRange& range = args.ranges[blockIdx.y / args.n_run_slices];
   if (range.code_map == nullptr) {
      return;  // (uniform) nothing is derived in this store
   }
   const uint32_t run_begin = range.run_slice_first[slice];
   const uint32_t run_end = range.run_slice_first[slice + 1];
   if (run_begin + blockIdx.x * (DERIVED_THREADS * RUNS_IN_FLIGHT) >= run_end) {
      return;  // (uniform) no chunk of runs for this block
   }
   // the slice's runs are dealt to the gridDim.x blocks of the slice in chunks of RUNS_IN_FLIGHT x 1024; a chunk's loads are
   // in flight together, and the next chunk's while this one is counted (the first beside the filter slice)
   const uint32_t chunk_runs = DERIVED_THREADS * RUNS_IN_FLIGHT;
   const auto loadRuns = [&](uint64_t (&key)[RUNS_IN_FLIGHT], uint32_t (&run_last)[RUNS_IN_FLIGHT], uint32_t base) {
#pragma unroll
      for (uint32_t k = 0; k < RUNS_IN_FLIGHT; ++k) {
         const uint32_t i = base + k * DERIVED_THREADS + threadIdx.x;
         key[k] = i < run_end ? range.run_keys[i] : 0;
         run_last[k] = i < run_end ? range.run_ends[i] : 0;  // (an empty run: start >= end below)
      }
   };
   uint64_t any_bit = 0;
   ulonglong2 filter_part[ESCAPE_SLICE_WORDS32 / 4u / DERIVED_THREADS];
   {
      const uint64_t* filter = args.filters[q];
      const uint32_t first_word = slice * (ESCAPE_SLICE_WORDS32 / 2u);
#pragma unroll
      for (uint32_t j = 0; j < ESCAPE_SLICE_WORDS32 / 4u / DERIVED_THREADS; ++j) {
         const uint32_t word = first_word + (j * DERIVED_THREADS + threadIdx.x) * 2u;  // 16-byte chunk of the slice
         filter_part[j] = word < args.row_words ? *reinterpret_cast<const ulonglong2*>(filter + word) : make_ulonglong2(0, 0);
      }
   }
   uint64_t next_key[RUNS_IN_FLIGHT];
   uint32_t next_last[RUNS_IN_FLIGHT];
   loadRuns(next_key, next_last, run_begin + blockIdx.x * chunk_runs);
   const uint32_t n = range.n_positions;
   if constexpr (LDS_DIFF) {
      for (uint32_t j = threadIdx.x * 4u; j <= n; j += DERIVED_THREADS * 4u) {  // (16 bytes per store; the array is rounded up to them)
         *reinterpret_cast<uint4*>(s_diff + j) = make_uint4(0, 0, 0, 0);
      }
   }
#pragma unroll
   for (uint32_t j = 0; j < ESCAPE_SLICE_WORDS32 / 4u / DERIVED_THREADS; ++j) {
      *reinterpret_cast<ulonglong2*>(s_runs + (j * DERIVED_THREADS + threadIdx.x) * 4u) = filter_part[j];
      any_bit |= filter_part[j].x | filter_part[j].y;
   }
   if (__syncthreads_or(any_bit != 0 ? 1 : 0) == 0) {
      return;  // no row of this slice is selected
   }
   uint32_t* __restrict__ diff = range.scratch + static_cast<size_t>(q) * range.stride + range.gaps_offset;
   const uint32_t slice_first_row = slice << ESCAPE_SLICE_SHIFT;
   const uint32_t pos_end = range.pos_begin + n;
   uint32_t from_the_first = 0;  // selected runs that begin at or before the range's first position (sequences that begin with the missing symbol: every lane on one counter otherwise)
   for (uint32_t base = run_begin + blockIdx.x * chunk_runs; base < run_end; base += gridDim.x * chunk_runs) {
      uint64_t key[RUNS_IN_FLIGHT];
      uint32_t run_last[RUNS_IN_FLIGHT];
#pragma unroll
      for (uint32_t k = 0; k < RUNS_IN_FLIGHT; ++k) {
         key[k] = next_key[k];
         run_last[k] = next_last[k];
      }
      if (base + gridDim.x * chunk_runs < run_end) {  // (uniform)
         loadRuns(next_key, next_last, base + gridDim.x * chunk_runs);
      }
#pragma unroll
      for (uint32_t k = 0; k < RUNS_IN_FLIGHT; ++k) {
         const uint32_t local = (static_cast<uint32_t>(key[k] >> 32) - slice_first_row) & ((1u << ESCAPE_SLICE_SHIFT) - 1u);
         const bool selected = ((s_runs[local >> 5] >> (local & 31u)) & 1u) != 0;
         const uint32_t start = max(static_cast<uint32_t>(key[k]), range.pos_begin);
         const uint32_t end = min(run_last[k], pos_end);
         if (selected && start < end) {
            if (start == range.pos_begin) {
               from_the_first += 1;
            } else if constexpr (LDS_DIFF) {
               atomicAdd(&s_diff[start - range.pos_begin], 1u);
            } else {
               atomicAdd(&diff[start - range.pos_begin], 1u);
            }
            if (end < pos_end) {  // (the entry behind the last position is never summed)
               if constexpr (LDS_DIFF) {
                  atomicAdd(&s_diff[end - range.pos_begin], 0xFFFFFFFFu);
               } else {
                  atomicAdd(&diff[end - range.pos_begin], 0xFFFFFFFFu);
               }
            }
         }
      }
   }
   from_the_first = waveSumToLane63(from_the_first);
   if ((threadIdx.x & 63u) == 63u && from_the_first != 0) {
      if constexpr (LDS_DIFF) {
         atomicAdd(&s_diff[0], from_the_first);
      } else {
         atomicAdd(&diff[0], from_the_first);
      }
   }
   if constexpr (LDS_DIFF) {
      // The block's diff leaves as a part of its own, in plain 16-byte stores; k_sum_run_parts adds the parts up.  (Adding it
      // to the range's diff with atomics from here — 231 blocks x 30 000 entries at 10 M rows, device-scope atomics are
      // performed at the memory side — took 30 of this kernel's 43 us: profiles/r03_notes.md.)
      __syncthreads();
      const uint32_t part = ((q * args.n_ranges + blockIdx.y / args.n_run_slices) * args.n_run_slices + slice) * gridDim.x + blockIdx.x;
      uint32_t* __restrict__ out = args.run_parts + static_cast<size_t>(part) * args.part_stride;
      for (uint32_t j = threadIdx.x * 4u; j <= n; j += DERIVED_THREADS * 4u) {
         *reinterpret_cast<uint4*>(out + j) = *reinterpret_cast<const uint4*>(s_diff + j);
      }
      if (threadIdx.x == 0) {
         args.run_flags[part] = 1u;
      }
   }
}

/// diff[j] of a range and filter += the parts of the blocks of k_scan_missing_runs that raised their flag.  grid = (blocks of
/// 1024 entries, range x RUN_PART_GROUPS, filter): a thread owns 4 consecutive entries and a group of parts.
constexpr uint32_t RUN_PART_GROUPS = 16;
__global__ __launch_bounds__(256) void k_sum_run_parts(const DerivedArgs args) {
   const uint32_t q = blockIdx.z;
   const uint32_t r = blockIdx.y / RUN_PART_GROUPS;
   const uint32_t group = blockIdx.y % RUN_PART_GROUPS;
   const DerivedRange& range = args.ranges[r];
   const uint32_t n = range.n_positions;
   const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 4u;
   if (range.code_map == nullptr || blockIdx.x * 1024u > n) {
      return;  // (uniform)
   }
   const uint32_t parts_of_range = args.n_run_slices * args.run_blocks_per_slice;
   const uint32_t per_group = (parts_of_range + RUN_PART_GROUPS - 1) / RUN_PART_GROUPS;
   const uint32_t first = (q * args.n_ranges + r) * parts_of_range;
   const uint32_t begin = first + group * per_group;
   const uint32_t end = min(begin + per_group, first + parts_of_range);
   const uint32_t j_safe = j <= n ? j : 0;
   uint4 sum = make_uint4(0, 0, 0, 0);
   for (uint32_t part = begin; part < end; part += 8) {  // (uniform) eight parts' loads in flight
      uint4 v[8];
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
         v[k] = make_uint4(0, 0, 0, 0);
         if (part + k < end && args.run_flags[part + k] != 0) {
            v[k] = *reinterpret_cast<const uint4*>(args.run_parts + static_cast<size_t>(part + k) * args.part_stride + j_safe);
         }
      }
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
         sum.x += v[k].x;
         sum.y += v[k].y;
         sum.z += v[k].z;
         sum.w += v[k].w;
      }
   }
   if (j > n) {
      return;
   }
   uint32_t* __restrict__ diff = range.scratch + static_cast<size_t>(q) * range.stride + range.gaps_offset;
   const uint32_t values[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
   for (uint32_t c = 0; c < 4; ++c) {
      if (values[c] != 0 && j + c <= n) {
         atomicAdd(&diff[j + c], values[c]);
      }
   }
}

/// ambiguous[p] += the rows of filter blockIdx.y among the sparse keys (ambiguity codes) of position p: one global filter
/// lookup per key (these are ~1e-5 of the cells), one atomic per distinct position and wave.
__global__ __launch_bounds__(256) void k_count_sparse_keys(const DerivedArgs args) {
   const uint32_t q = blockIdx.y;
   const uint32_t lane = threadIdx.x & 63u;
   uint32_t r = 0;
   while (r + 1 < args.n_ranges && blockIdx.x >= args.first_unit[r + 1]) {
      ++r;
   }
   const DerivedRange& range = args.ranges[r];
   const uint32_t n = range.n_positions;
   uint32_t* __restrict__ ambiguous = range.scratch + static_cast<size_t>(q) * range.stride + range.gaps_offset + n + 1u;
   const uint32_t first = range.sparse_begin + (blockIdx.x - args.first_unit[r]) * (256u * SPARSE_KEYS_PER_THREAD) + threadIdx.x;
   uint64_t key[SPARSE_KEYS_PER_THREAD];
#pragma unroll
   for (uint32_t k = 0; k < SPARSE_KEYS_PER_THREAD; ++k) {
      const uint32_t i = first + k * 256u;
      key[k] = i < range.sparse_end ? range.sparse_keys[i] : 0;
   }
   uint64_t word[SPARSE_KEYS_PER_THREAD];
#pragma unroll
   for (uint32_t k = 0; k < SPARSE_KEYS_PER_THREAD; ++k) {  // the filter lookups of all keys of the thread in flight together
      word[k] = args.filters[q][static_cast<uint32_t>(key[k]) >> 6];
   }
#pragma unroll
   for (uint32_t k = 0; k < SPARSE_KEYS_PER_THREAD; ++k) {
      const uint32_t sequence = static_cast<uint32_t>(key[k]);
      bool pending = first + k * 256u < range.sparse_end && ((word[k] >> (sequence & 63u)) & 1ull) != 0;
      const uint32_t counter = static_cast<uint32_t>(key[k] >> 37) - range.pos_begin;
      for (uint64_t open = __ballot(pending); open != 0; open = __ballot(pending)) {
         const uint32_t leader = static_cast<uint32_t>(__builtin_ctzll(open));
         const uint32_t leader_counter = __shfl(counter, leader);
         const uint64_t same = __ballot(pending && counter == leader_counter);
         if (lane == leader) {
            atomicAdd(&ambiguous[leader_counter], static_cast<uint32_t>(__popcll(same)));
         }
         if (counter == leader_counter) {
            pending = false;
         }
      }
   }
}

/// The last step of a scan with derived symbols: grid = (blocks of 1024 positions dealt to the ranges, filter).  A thread
/// owns a position: the rows of the filter inside a run of the missing symbol there (the sum of diff up to it: the part
/// before the block's positions summed by the block itself, then a scan over the block), plus those with an ambiguity code,
/// are the rows without a valid symbol; what is left of the filter after them and after the other symbols' counts is the
/// derived symbol's count.  The private table is added to the caller's.
/// EVENTS: the private table holds gaps[n][2] (the selected rows' gap events that start and end at a position) behind the
/// counts instead of diff and ambiguous; the rows without a valid symbol at p are the starts up to p less the ends up to p.
/// A range that counts the end runs of the gap symbol (DerivedRange::position_covered) has ends[n][2] behind that: at a covered
/// position the gap symbol's cell gets, on top of its residual keys, the selected rows inside an end run — |F| less the lead-end
/// events up to p plus the trail-start events up to p — before the derived count is formed; elsewhere ends is ignored.
/// SELECT (0, or the n_scan of every range of the launch; EVENTS only): the scan is the only writer of the caller's tables and
/// their only reader is the row selection of a Mutations query (silo_gpu_mutations_scan_select).  The thread then STORES every
/// cell of its position, zeros included, and applies K4's arithmetic (k_mutations_select_to_host) to the cells it holds: the
/// rows go straight into the filter's row slot, and the block that takes the last ticket of the scan's finish launches for
/// the filter publishes the header word.  No block waits for another.
constexpr uint32_t PREFIX_IN_FLIGHT = 4;  // 16-byte loads per array and thread in flight together in the sweep before the block's positions
template <bool EVENTS, uint32_t SELECT>
__global__ __launch_bounds__(DERIVED_THREADS) void k_finish_scan(const DerivedArgs args) {
   static_assert(SELECT == 0 || EVENTS, "the selection is fused into the finish of a scan that counts gap events");
   __shared__ uint32_t s_before[2][DERIVED_THREADS / 64];  // [0] the gaps, [1] the end runs
   __shared__ uint32_t s_own[2][DERIVED_THREADS / 64];
   const uint32_t q = blockIdx.y;
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t wave = threadIdx.x >> 6;
   uint32_t r = 0;
   while (r + 1 < args.n_ranges && blockIdx.x >= args.first_unit[r + 1]) {
      ++r;
   }
   const DerivedRange& range = args.ranges[r];
   const uint32_t n = range.n_positions;
   const uint32_t n_scan = SELECT != 0 ? SELECT : range.n_scan;
   const uint32_t first_position = (blockIdx.x - args.first_unit[r]) * DERIVED_THREADS;
   const uint32_t p = first_position + threadIdx.x;
   const uint32_t* __restrict__ counts = range.scratch + static_cast<size_t>(q) * range.stride;
   const uint32_t* __restrict__ diff = counts + range.gaps_offset;
   const uint32_t* __restrict__ ambiguous = diff + n + 1u;
   const auto diffAt = [&](uint32_t j) {  // rows entering less rows leaving the gaps at j
      if constexpr (EVENTS) {
         return diff[2u * j] - diff[2u * j + 1u];
      } else {
         return diff[j];
      }
   };
   // a range that counts end runs: trailing runs beginning less leading runs ending at j — summed up to p and added to |F|, the rows
   // of the filter inside an end run at p.  Both sums are taken in ONE sweep over the positions before the block's.  The sweep
   // was a chain of memory latencies (a 4-byte load per thread and turn, 29 turns in the genome's last block: 16.3 us); both
   // arrays are 16-byte aligned (gaps_offset, ends_offset) and first_position is a multiple of 1024, so a thread takes whole
   // uint4 — two positions of gaps or ends, four of diff — and has PREFIX_IN_FLIGHT of them per array in flight before the
   // first is consumed: 15 per array and thread at 29 903 positions, four turns.
   const bool with_ends = EVENTS && range.code_map != nullptr && range.position_covered != nullptr;  // (uniform)
   const uint32_t* __restrict__ ends = counts + range.ends_offset;
   const auto endAt = [&](uint32_t j) { return ends[2u * j + 1u] - ends[2u * j]; };
   uint32_t without_symbol = 0;  // rows of the filter that have no valid symbol at p
   uint32_t in_end_run = 0;      // rows of the filter inside a leading or trailing run of the gap symbol at p
   // What the thread needs of its own position besides the prefix sums depends on none of them: it is loaded here, ahead of the
   // sweep, so that these latencies pass beside the sweep's and not one after another behind the barrier (a finish launch is
   // 30 blocks: nothing else hides them).  Same guards as where the values are used.
   const bool has_map = range.code_map != nullptr;  // (uniform)
   const uint32_t filter_rows = has_map ? args.counters[q * SPARSE_COUNTER_STRIDE + 2] : 0u;  // |F|
   uint32_t map_flags = 0, map_slot = 0, covered_here = 0;
   if (p < n) {
      if (has_map) {
         const uint8_t* map = range.code_map + static_cast<size_t>(range.pos_begin + p) * CODE_MAP_STRIDE;
         map_flags = map[0];
         map_slot = map[IMPLICIT_SLOT];
      }
      covered_here = with_ends ? range.position_covered[range.pos_begin + p] : 0u;
   }
   // SELECT: the position's cells of the private table and the index of its reference symbol too.  The 22 cells of an amino-acid
   // position held across the sweep cost a wave per SIMD (66 VGPRs against 50): there the cells are loaded where they are used.
   constexpr bool CELLS_AHEAD = SELECT != 0 && SELECT <= 8;
   uint32_t held[SELECT != 0 ? SELECT : 1] = {};
   uint32_t reference = 0;
   const auto loadCells = [&]() {
      const uint32_t* __restrict__ cell = counts + static_cast<size_t>(p) * SELECT;
#pragma unroll
      for (uint32_t symbol = 0; symbol < SELECT; ++symbol) {
         held[symbol] = cell[symbol];
      }
   };
   if constexpr (SELECT != 0) {
      if (p < n) {
         if constexpr (CELLS_AHEAD) {
            loadCells();
         }
         reference = args.sinks[q].reference_index[range.table_offset + p];
      }
   }
   if (has_map) {  // (uniform)
      uint32_t before[2] = {0, 0};
      const uint4* __restrict__ diff16 = reinterpret_cast<const uint4*>(diff);
      const uint4* __restrict__ ends16 = reinterpret_cast<const uint4*>(ends);
      uint32_t own[2] = {0u, 0u};
      if (p < n) {  // (one guard for both, so that the two loads leave together and are waited for once)
         own[0] = diffAt(p);
         own[1] = with_ends ? endAt(p) : 0u;
      }
      const uint32_t n16 = EVENTS ? first_position / 2u : first_position / 4u;  // (exact: first_position is a multiple of 1024)
      for (uint32_t base = 0; base < n16; base += DERIVED_THREADS * PREFIX_IN_FLIGHT) {  // (uniform)
         uint4 d[PREFIX_IN_FLIGHT];
         uint4 e[PREFIX_IN_FLIGHT];
#pragma unroll
         for (uint32_t k = 0; k < PREFIX_IN_FLIGHT; ++k) {
            const uint32_t i = base + k * DERIVED_THREADS + threadIdx.x;
            d[k] = i < n16 ? diff16[i] : make_uint4(0, 0, 0, 0);
            e[k] = with_ends && i < n16 ? ends16[i] : make_uint4(0, 0, 0, 0);
         }
#pragma unroll
         for (uint32_t k = 0; k < PREFIX_IN_FLIGHT; ++k) {
            before[0] += EVENTS ? d[k].x - d[k].y + d[k].z - d[k].w : d[k].x + d[k].y + d[k].z + d[k].w;
            before[1] += e[k].y - e[k].x + e[k].w - e[k].z;
         }
      }
      const uint32_t scanned[2] = {waveSumToLane63(own[0]), waveSumToLane63(own[1])};  // inclusive over the wave
#pragma unroll
      for (int t = 0; t < 2; ++t) {
         before[t] = waveSumToLane63(before[t]);
         if (lane == 63u) {
            s_before[t][wave] = before[t];
            s_own[t][wave] = scanned[t];
         }
      }
      __syncthreads();
      without_symbol = scanned[0];
      in_end_run = scanned[1];
      for (uint32_t k = 0; k < DERIVED_THREADS / 64; ++k) {
         without_symbol += s_before[0][k] + (k < wave ? s_own[0][k] : 0u);
         in_end_run += s_before[1][k] + (k < wave ? s_own[1][k] : 0u);
      }
      if (!EVENTS && p < n) {
         without_symbol += ambiguous[p];
      }
      in_end_run += filter_rows;
   }
   // (the bytes stay as loaded until here: left alone, the compiler tests them right behind their loads, which waits for each
   // of them ahead of the sweep instead of beside it)
   asm volatile("" : "+v"(map_flags), "+v"(map_slot), "+v"(covered_here));
   if constexpr (SELECT == 0) {
      if (p >= n) {
         return;
      }
      if (covered_here == 0) {  // only the covered positions take their gap rows from the end runs: everywhere else the row was read
         in_end_run = 0;
      }
      uint32_t* __restrict__ out = range.caller_counts[q] + static_cast<size_t>(p) * n_scan;
      const uint32_t* __restrict__ cell = counts + static_cast<size_t>(p) * n_scan;
      uint32_t others = 0;
      for (uint32_t symbol = 0; symbol < n_scan; ++symbol) {
         const uint32_t count = cell[symbol] + (symbol == range.end_symbol ? in_end_run : 0u);
         others += count;
         if (count != 0) {
            out[symbol] += count;  // scans of one table are ordered on a stream: no atomic needed
         }
      }
      if ((map_flags & LAYOUT_IMPLICIT) != 0) {  // (0 without a code map)
         const uint32_t derived = filter_rows - without_symbol - others;
         if (derived != 0) {
            out[map_slot] += derived;
         }
      }
   } else {
      const SelectSink& sink = args.sinks[q];
      uint32_t selected = 0;  // bit s: symbol s passes
      if (p < n) {
         if (covered_here == 0) {
            in_end_run = 0;
         }
         if constexpr (!CELLS_AHEAD) {
            loadCells();
         }
         uint32_t count[SELECT];
         uint32_t others = 0;
#pragma unroll
         for (uint32_t symbol = 0; symbol < SELECT; ++symbol) {
            count[symbol] = held[symbol] + (symbol == range.end_symbol ? in_end_run : 0u);
            others += count[symbol];
         }
         uint32_t covered = others;  // the sum of the position's final cells (uint32 wrap-around as in K4)
         if ((map_flags & LAYOUT_IMPLICIT) != 0) {  // (0 without a code map)
            const uint32_t derived = filter_rows - without_symbol - others;
#pragma unroll
            for (uint32_t symbol = 0; symbol < SELECT; ++symbol) {
               count[symbol] += symbol == map_slot ? derived : 0u;
            }
            covered += derived;
         }
         uint32_t* __restrict__ out = range.caller_counts[q] + static_cast<size_t>(p) * SELECT;
#pragma unroll
         for (uint32_t symbol = 0; symbol < SELECT; ++symbol) {
            out[symbol] = count[symbol];  // the only writer of the cell: whatever the table held is gone
         }
         // K4 (k_mutations_select_to_host) on the cells at hand
         const uint32_t position = range.table_offset + p;
         if (covered != 0) {
            const uint32_t threshold_count =
               sink.min_proportion == 0 ? 0u : static_cast<uint32_t>(ceil(static_cast<double>(covered) * sink.min_proportion) - 1);
#pragma unroll
            for (uint32_t symbol = 0; symbol < SELECT; ++symbol) {
               if (symbol != reference && count[symbol] > threshold_count) {
                  selected |= 1u << symbol;
               }
            }
         }
         if (selected != 0) {
            uint32_t slot = atomicAdd(&sink.cursor_and_ticket[0], static_cast<uint32_t>(__popc(selected)));
#pragma unroll
            for (uint32_t symbol = 0; symbol < SELECT; ++symbol) {
               if ((selected >> symbol) & 1u) {
                  if (slot < sink.capacity) {
                     sink.host_rows[slot] = silo_gpu_mutation_row{position, symbol, count[symbol], covered};
                  }
                  ++slot;
               }
            }
         }
      }
      // Only a thread that stored a row has anything to make visible to the host, so only it pays for a system-scope fence:
      //   - a row's stores are fenced by their writer, before that writer reaches the barrier;
      //   - thread 0 takes the block's ticket after the barrier, so after every fence of the block;
      //   - the holder of the last ticket has seen every other block's ticket, each taken after that block's fences, and
      //     publishes the header with a system-scope release.
      // The host reads rows only after it has read the header.  A block without a selected row takes its ticket with no fence at all.
      if (selected != 0) {
         __threadfence_system();
      }
      __syncthreads();
      if (threadIdx.x == 0) {
         if (atomicAdd(&sink.cursor_and_ticket[1], 1u) == sink.total_blocks - 1) {  // the last block of the scan's finish launches for this filter
            const uint32_t n_selected = atomicExch(&sink.cursor_and_ticket[0], 0u);
            atomicExch(&sink.cursor_and_ticket[1], 0u);
            __hip_atomic_store(sink.host_header, (static_cast<unsigned long long>(sink.epoch) << 32) | n_selected, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
         }
      }
   }
}

/// Blocks per slice of k_scan_missing_runs: one block per CU fits (its LDS), about one round of the 256 CUs over all (slice, range, filter).
uint32_t runBlocksPerSlice(const DerivedArgs& launch, uint32_t q_count) {
   const uint32_t run_units = std::max<uint32_t>(1, launch.n_run_slices * launch.n_ranges * q_count);
   return std::min<uint32_t>(8, std::max<uint32_t>(1, 240 / run_units));
}

/// Does a scan of `range` count the end runs of the gap symbol instead of reading its covered rows?  The store has them, the knob
/// (SILO_GPU_TUNE_END_RUNS, read once per scan) allows it, and every run of one-hot rows of the range fits the row kernel's list of live rows.
bool usesEndRuns(const ScanRange& range, int knob) {
   const SeqStoreHost::Layout& layout = range.seqstore->layout;
   if (layout.ends.d_keys.get() == nullptr || layout.d_row_covered.get() == nullptr || knob < 0) {
      return false;
   }
   for (const SeqStoreHost::Run& run : layout.runs) {
      const uint32_t begin = std::max(run.begin, range.pos_begin);
      const uint32_t end = std::min(run.end, range.pos_end);
      if (run.one_hot && begin < end && layout.row_of[end] - layout.row_of[begin] > ROW_LIST_MAX) {
         return false;
      }
   }
   return true;
}

}  // namespace

namespace silo_gpu_detail {

/// Does a scan of `ranges` count the gap events of its stores (DerivedPlan::events)?  The knobs allow it and every store with
/// derived symbols has them.
bool derivedCountsEvents(const std::vector<ScanRange>& ranges) {
   bool events = g_tune_gap_events.load() >= 0 && g_tune_side_stream.load() != 3;
   for (const ScanRange& range : ranges) {
      events = events && (!range.seqstore->layout.has_implicit || range.seqstore->layout.gap_stream);
   }
   return events;
}

/// Lays the private tables of `ranges` out (offsets only: `tables` may still be null).  `select` (or nullptr): the finish
/// launches overwrite the callers' tables and deliver the selected rows (the caller has checked that the scan counts gap events).
void planDerived(const silo_gpu_store* store, const std::vector<ScanRange>& ranges, const uint64_t* const* filters, uint32_t q_count, DerivedPlan& plan,
   const ScanSelect* select) {
   plan.private_ranges = ranges;
   plan.launches.assign((ranges.size() + DERIVED_MAX_RANGES - 1) / DERIVED_MAX_RANGES, DerivedArgs{});
   plan.run_counts.assign(plan.launches.size(), {});
   plan.events = derivedCountsEvents(ranges);
   plan.select = select != nullptr && plan.events;
   if (plan.select) {
      std::vector<uint32_t> n_positions;
      for (const ScanRange& range : ranges) {
         n_positions.push_back(range.pos_end - range.pos_begin);
      }
      const uint32_t total_blocks = finishBlocks(n_positions.data(), n_positions.size(), DERIVED_THREADS);
      for (DerivedArgs& launch : plan.launches) {
         std::copy_n(select->sinks, q_count, launch.sinks);
         for (uint32_t q = 0; q < q_count; ++q) {
            launch.sinks[q].total_blocks = total_blocks;
         }
      }
   }
   plan.gap_ranges.assign(plan.events ? ranges.size() : 0, ScanRange{});
   const int end_knob = g_tune_end_runs.load();
   plan.ends_apart = end_knob == 1;
   plan.end_runs.assign(ranges.size(), 0);
   plan.end_ranges.assign(ranges.size(), ScanRange{});
   size_t offset = 0;
   for (size_t r = 0; r < ranges.size(); ++r) {
      const ScanRange& range = ranges[r];
      const SeqStoreHost& seqstore = *range.seqstore;
      DerivedArgs& launch = plan.launches[r / DERIVED_MAX_RANGES];
      DerivedRange& entry = launch.ranges[launch.n_ranges++];
      const uint32_t n = range.pos_end - range.pos_begin;
      entry.n_positions = n;
      entry.n_scan = seqstore.dev.n_scan;
      entry.pos_begin = range.pos_begin;
      entry.table_offset = plan.select ? select->table_offset[r] : 0;
      // counts[n][n_scan], then gaps[n][2] (the events: starts, ends) — and ends[n][2] where the range counts end runs — or
      // diff[n + 1] and ambiguous[n]; gaps / diff and ends begin at a multiple of 16 bytes (the sweep of k_finish_scan)
      const bool end_runs = plan.events && seqstore.layout.has_implicit && usesEndRuns(range, end_knob);
      plan.end_runs[r] = end_runs ? 1 : 0;
      entry.position_covered = end_runs ? seqstore.layout.d_position_covered.get() : nullptr;
      entry.end_symbol = seqstore.layout.end_symbol;
      const auto rounded = [](size_t words) { return (words + 3) / 4 * 4; };
      const size_t gaps_offset = rounded(static_cast<size_t>(n) * seqstore.dev.n_scan);
      const size_t ends_offset = rounded(gaps_offset + 2 * static_cast<size_t>(n));
      entry.gaps_offset = static_cast<uint32_t>(gaps_offset);
      entry.ends_offset = static_cast<uint32_t>(ends_offset);
      entry.stride = static_cast<uint32_t>(rounded(plan.events ? ends_offset + (end_runs ? 2 * static_cast<size_t>(n) : 0) : gaps_offset + n + 1 + n));
      entry.scratch = reinterpret_cast<uint32_t*>(offset * sizeof(uint32_t));  // + the scratch block's tables (bindDerived)
      offset += static_cast<size_t>(entry.stride) * q_count;
      if (seqstore.layout.has_implicit) {
         plan.run_counts[r / DERIVED_MAX_RANGES][launch.n_ranges - 1] = seqstore.dev.n_missing_runs;
         entry.code_map = seqstore.layout.d_code_map.get();
         entry.run_keys = seqstore.dev.missing_run_keys;
         entry.run_ends = seqstore.dev.missing_run_ends;
         entry.run_slice_first = seqstore.layout.d_run_slice_first.get();
         launch.n_run_slices = seqstore.layout.n_run_slices;
         entry.sparse_keys = seqstore.d_sparse.get();
         const auto lo = std::lower_bound(seqstore.sparse_sorted.begin(), seqstore.sparse_sorted.end(), static_cast<uint64_t>(range.pos_begin) << 37);
         const auto hi = std::lower_bound(lo, seqstore.sparse_sorted.end(), static_cast<uint64_t>(range.pos_end) << 37);
         entry.sparse_begin = static_cast<uint32_t>(lo - seqstore.sparse_sorted.begin());
         entry.sparse_end = static_cast<uint32_t>(hi - seqstore.sparse_sorted.begin());
         plan.most_positions = std::max(plan.most_positions, n);
      }
      std::copy_n(range.counts, q_count, entry.caller_counts);
      copyFilters(launch.filters, filters, q_count);
      launch.row_words = store->row_words;
   }
   if (plan.events) {  // no run parts
      plan.table_words = offset;
      return;
   }
   // the parts of the blocks of k_scan_missing_runs: flags in the zeroed area, the parts behind it (offsets until bindDerived)
   const uint32_t part_stride = (plan.most_positions + 4) / 4 * 4;
   size_t part_offset = 0;
   for (DerivedArgs& launch : plan.launches) {
      launch.run_blocks_per_slice = runBlocksPerSlice(launch, q_count);
      launch.part_stride = part_stride;
      const size_t parts = static_cast<size_t>(q_count) * launch.n_ranges * launch.n_run_slices * launch.run_blocks_per_slice;
      launch.run_flags = reinterpret_cast<uint32_t*>(offset * sizeof(uint32_t));
      offset += (parts + 3) / 4 * 4;
      launch.run_parts = reinterpret_cast<uint32_t*>(part_offset * sizeof(uint32_t));
      part_offset += parts * part_stride;
   }
   plan.table_words = offset;
   plan.part_words = part_offset;
}

/// The tables get their place in the scratch block (`tables`; `counters`: the prepare step's); the private ranges point at them.
void bindDerived(DerivedPlan& plan, uint32_t* tables, const uint32_t* counters, uint32_t q_count) {
   size_t r = 0;
   for (DerivedArgs& launch : plan.launches) {
      launch.counters = counters;
      if (!plan.events) {
         launch.run_flags = tables + reinterpret_cast<size_t>(launch.run_flags) / sizeof(uint32_t);
         launch.run_parts = tables + plan.table_words + reinterpret_cast<size_t>(launch.run_parts) / sizeof(uint32_t);
      }
      for (uint32_t k = 0; k < launch.n_ranges; ++k, ++r) {
         DerivedRange& entry = launch.ranges[k];
         entry.scratch = tables + reinterpret_cast<size_t>(entry.scratch) / sizeof(uint32_t);
         for (uint32_t q = 0; q < q_count; ++q) {
            plan.private_ranges[r].counts[q] = entry.scratch + static_cast<size_t>(q) * entry.stride;
         }
         if (plan.events && entry.code_map != nullptr) {
            ScanRange& gap = plan.gap_ranges[r];
            gap = plan.private_ranges[r];
            for (uint32_t q = 0; q < q_count; ++q) {
               gap.counts[q] = entry.scratch + static_cast<size_t>(q) * entry.stride + entry.gaps_offset;
            }
         }
         if (plan.end_runs[r] != 0) {
            ScanRange& end = plan.end_ranges[r];
            end = plan.private_ranges[r];
            for (uint32_t q = 0; q < q_count; ++q) {
               end.counts[q] = entry.scratch + static_cast<size_t>(q) * entry.stride + entry.ends_offset;
            }
         }
      }
   }
}

/// Rows of the filters without a valid symbol, per position: the runs of the missing symbol and the sparse keys (ambiguity codes).
int scanRowsWithoutSymbol(DerivedPlan& plan, uint32_t q_count, hipStream_t hip_stream) {
   for (DerivedArgs& launch : plan.launches) {
      bool any = false;
      for (uint32_t k = 0; k < launch.n_ranges; ++k) {
         any = any || launch.ranges[k].code_map != nullptr;
      }
      if (!any) {
         continue;
      }
      // the diff of a range in LDS beside the filter slice, while it fits
      const size_t lds_bytes = (ESCAPE_SLICE_WORDS32 + (static_cast<size_t>(plan.most_positions) + 4) / 4 * 4) * sizeof(uint32_t);
      const bool lds_diff = lds_bytes <= 152 * 1024;
      static std::once_flag lds_once;
      std::call_once(lds_once, [] {
         (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_scan_missing_runs<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
      });
      const dim3 run_grid(launch.run_blocks_per_slice, launch.n_run_slices * launch.n_ranges, q_count);
      uint64_t run_bytes = 0, sparse_bytes = 0;
      for (uint32_t k = 0; k < launch.n_ranges; ++k) {
         if (launch.ranges[k].code_map != nullptr) {
            run_bytes += plan.run_counts[&launch - plan.launches.data()][k] * (sizeof(uint64_t) + sizeof(uint32_t));
            sparse_bytes += static_cast<uint64_t>(launch.ranges[k].sparse_end - launch.ranges[k].sparse_begin) * sizeof(uint64_t);
         }
      }
      ScanLaunchTiming* run_timing = startLaunchTiming(lds_diff ? "k_scan_missing_runs<true>" : "k_scan_missing_runs<false>", 0, run_bytes * q_count, q_count, run_grid.x * run_grid.y * run_grid.z, hip_stream);
      if (lds_diff) {
         k_scan_missing_runs<true><<<run_grid, DERIVED_THREADS, lds_bytes, hip_stream>>>(launch);
         k_sum_run_parts<<<dim3(plan.most_positions / 1024 + 1, launch.n_ranges * RUN_PART_GROUPS, q_count), 256, 0, hip_stream>>>(launch);
      } else {
         k_scan_missing_runs<false><<<run_grid, DERIVED_THREADS, ESCAPE_SLICE_WORDS32 * sizeof(uint32_t), hip_stream>>>(launch);
      }
      HIP_TRY(hipGetLastError());
      finishLaunchTiming(run_timing, hip_stream);
      launch.first_unit[0] = 0;
      for (uint32_t k = 0; k < launch.n_ranges; ++k) {
         const uint32_t keys = launch.ranges[k].code_map != nullptr ? launch.ranges[k].sparse_end - launch.ranges[k].sparse_begin : 0;
         launch.first_unit[k + 1] = launch.first_unit[k] + (keys + 256 * SPARSE_KEYS_PER_THREAD - 1) / (256 * SPARSE_KEYS_PER_THREAD);
      }
      if (launch.first_unit[launch.n_ranges] != 0) {
         ScanLaunchTiming* sparse_timing = startLaunchTiming("k_count_sparse_keys", 0, sparse_bytes * q_count, q_count, launch.first_unit[launch.n_ranges] * q_count, hip_stream);
         k_count_sparse_keys<<<dim3(launch.first_unit[launch.n_ranges], q_count), 256, 0, hip_stream>>>(launch);
         HIP_TRY(hipGetLastError());
         finishLaunchTiming(sparse_timing, hip_stream);
      }
   }
   return SILO_GPU_OK;
}

/// The derived counts, and the private tables into the caller's.
int finishDerived(DerivedPlan& plan, uint32_t q_count, hipStream_t hip_stream) {
   for (DerivedArgs& launch : plan.launches) {
      launch.first_unit[0] = 0;
      for (uint32_t k = 0; k < launch.n_ranges; ++k) {
         launch.first_unit[k + 1] = launch.first_unit[k] + (launch.ranges[k].n_positions + DERIVED_THREADS - 1) / DERIVED_THREADS;
      }
      if (launch.first_unit[launch.n_ranges] != 0) {
         const dim3 grid(launch.first_unit[launch.n_ranges], q_count);
         const bool nucleotide = launch.ranges[0].n_scan == 5;  // (a scan's ranges are of one alphabet)
         uint64_t table_bytes = 0;  // the private tables: every word read once
         for (uint32_t k = 0; k < launch.n_ranges; ++k) {
            table_bytes += static_cast<uint64_t>(launch.ranges[k].stride) * q_count * sizeof(uint32_t);
         }
         // (the instantiation is named in the timing log: whether a scan selected its rows here is not visible in its tables)
         const char* const name = plan.select ? (nucleotide ? "k_finish_scan<true, 5>" : "k_finish_scan<true, 22>")
                                              : (plan.events ? "k_finish_scan<true, 0>" : "k_finish_scan<false, 0>");
         ScanLaunchTiming* timing = startLaunchTiming(name, 0, table_bytes, q_count, grid.x * grid.y, hip_stream);
         if (plan.select && nucleotide) {
            k_finish_scan<true, 5><<<grid, DERIVED_THREADS, 0, hip_stream>>>(launch);
         } else if (plan.select) {
            k_finish_scan<true, 22><<<grid, DERIVED_THREADS, 0, hip_stream>>>(launch);
         } else if (plan.events) {
            k_finish_scan<true, 0><<<grid, DERIVED_THREADS, 0, hip_stream>>>(launch);
         } else {
            k_finish_scan<false, 0><<<grid, DERIVED_THREADS, 0, hip_stream>>>(launch);
         }
         HIP_TRY(hipGetLastError());
         finishLaunchTiming(timing, hip_stream);
      }
   }
   return SILO_GPU_OK;
}

}  // namespace silo_gpu_detail
