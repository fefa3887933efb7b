// silo_gpu_scan_keys.hip — the escape keys of K1, the Mutations scan ("The escape pass", "Keys that cannot reach
// minProportion"): the rows the plane rows do not carry, one key per (position, symbol, sequence); and, in the same launches, the
// gap events of a store with derived symbols and — where a range counts them — the end events of the gap symbol and the residual
// keys of its covered rows ("The gap symbol's end runs instead of its rows").
//
// Kernels:
//   k_scan_escapes_sliced<FILTERS, WALK>   the slice-major 4-byte keys against a slice of 1, 2, 4 or 8 filters in LDS; a block per item, or blocks that walk the items
//   k_scan_escapes_overflow          the few keys that do not fit the packed form
//   k_scan_escapes                   the position-major 8-byte keys (stores of more than 512 slices; an independent check)
// Exported (scan_internal.h): scanEscapes.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "escape_item_plan.h"
#include "scan_internal.h"

using namespace silo_gpu_detail;

namespace {

/// The rows the code planes do not carry: one key per (position, symbol, sequence); grid.y = filter.  A thread takes
/// ESCAPE_KEYS_PER_THREAD keys a block-width apart (their loads and the filter lookups behind them are in flight together).
constexpr uint32_t ESCAPE_KEYS_PER_THREAD = 4;
__global__ __launch_bounds__(256) void k_scan_escapes(
   const uint64_t* __restrict__ escapes, uint32_t n_escapes, const ScanBatchArgs batch, uint32_t pos_begin
) {
   const uint32_t q = blockIdx.y;  // every filter: dense scan and sparse-filter gather of a range both read the same planes
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t first = blockIdx.x * (256u * ESCAPE_KEYS_PER_THREAD) + threadIdx.x;
   uint64_t key[ESCAPE_KEYS_PER_THREAD];
   bool selected[ESCAPE_KEYS_PER_THREAD];
#pragma unroll
   for (uint32_t k = 0; k < ESCAPE_KEYS_PER_THREAD; ++k) {
      const uint32_t i = first + k * 256u;
      key[k] = i < n_escapes ? escapes[i] : 0;
   }
#pragma unroll
   for (uint32_t k = 0; k < ESCAPE_KEYS_PER_THREAD; ++k) {
      const uint32_t sequence = static_cast<uint32_t>(key[k]);
      selected[k] = first + k * 256u < n_escapes && ((batch.filters[q][sequence >> 6] >> (sequence & 63u)) & 1ull) != 0;
   }
#pragma unroll
   for (uint32_t k = 0; k < ESCAPE_KEYS_PER_THREAD; ++k) {
      bool pending = selected[k];
      // keys of one position sit together and share a few symbols: one atomic per distinct counter and wave, not per key
      const uint32_t counter = (static_cast<uint32_t>(key[k] >> 37) - pos_begin) * batch.out_symbols + (static_cast<uint32_t>(key[k] >> 32) & 31u);
      for (uint64_t open = __ballot(pending); open != 0; open = __ballot(pending)) {
         const uint32_t leader = static_cast<uint32_t>(__builtin_ctzll(open));
         const uint32_t leader_counter = __shfl(counter, leader);
         const uint64_t same = __ballot(pending && counter == leader_counter);
         if (lane == leader) {
            atomicAdd(&batch.counts[0][q][leader_counter], static_cast<uint32_t>(__popcll(same)));
         }
         if (counter == leader_counter) {
            pending = false;
         }
      }
   }
}

/// One launch for up to ESCAPE_MAX_RANGES position ranges (the 12 genes of an AminoAcidMutations query), each over the
/// escape keys or the gap events of its store.  The work is numbered as ITEMS — every range items_per_slice per slice, slice by
/// slice, the ranges that are never pruned first (escape_item_plan.h) —; grid = (blocks that walk the items in turn, 1,
/// filters / FILTERS); where a slice's keys of the scanned positions begin and end is read from the store's slice index on the
/// device.
struct EscapeSliceArgs {
   const uint64_t* filters[SILO_GPU_MAX_SCAN_BATCH];
   uint32_t row_words;
   uint32_t n_slices;
   uint32_t n_ranges;
   uint32_t block_keys;  // keys of an item's share: whole granules, at most ESCAPE_GRANULES_PER_BLOCK
   uint32_t n_items;     // block b takes the items b, b + gridDim.x, ... below it
   // a scan that may leave out keys no Mutations row can come from (silo_gpu_mutations_scan_ranges_min_proportion): the counters of
   // the prepare step ([q * SPARSE_COUNTER_STRIDE + 2] = the cardinality of filter q) and every filter's proportion; a range
   // with bounds per granule (heaviest, without) skips the granules that granulePrunable() names for EVERY filter of the pass
   const uint32_t* counters;
   double min_proportion[SILO_GPU_MAX_SCAN_BATCH];
   struct Range {
      const uint32_t* keys;          // the packed slice-major keys of the store (a SliceMajorKeys of SeqStoreHost::Layout: escapes_sliced, gaps, ends or residual)
      const uint32_t* granule_base;  // counter of every granule's first key
      const uint32_t* slice_first;   // [n_slices][positions + 1], in the packed numbering
      const uint32_t* heaviest;      // per granule (SeqStoreHost::Layout::d_granule_heaviest), or nullptr: every granule is counted
      const uint32_t* without;       // per granule (d_granule_without)
      uint32_t positions;
      uint32_t pos_begin;
      uint32_t pos_end;
      uint32_t out_symbols;       // counters per position: the store's scan symbols (keys), 2 (gap events: starts, ends)
      uint32_t key_from;          // the position whose keys a slice's are read from: pos_begin, or 0 for gap events, whose
                                  // events before pos_begin count on pos_begin's counters (a gap open there counts as begun)
      uint32_t first_item;        // the items of the ranges before
      uint32_t items_per_slice;
      uint32_t* counts[SILO_GPU_MAX_SCAN_BATCH];  // of the range's first position
   } ranges[ESCAPE_MAX_RANGES];
};

static_assert(sizeof(EscapeSliceArgs) + sizeof(uint32_t) <= 4096, "k_scan_escapes_sliced takes its arguments by value: the kernel-argument segment holds 4 KiB");

/// Workgroup barrier for data exchanged through LDS only: waits for the wave's LDS operations, NOT for its outstanding global
/// loads — __syncthreads() is also a fence and drains vmcnt(0), which would stall a block on the loads it has prefetched for
/// its next step at every barrier.
__device__ __forceinline__ void ldsBarrier() {
   asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

/// FILTERS = filters a block serves with ONE pass over its keys (1, 2, 4 or 8: a batch of 8 filters keeps 8 x 16 KiB of filter
/// slices in LDS and reads every key once, not once per filter); blockIdx.z = first filter / FILTERS.
///
/// Keys.  4 bytes each: row within the slice | (counter - counter of the granule's first key) << 17; a granule is 4 096
/// consecutive keys of a slice, so ONE 16-byte load per lane of the block fetches a granule, four consecutive keys per lane,
/// and the granule's base counter is a scalar.
///
/// Counting.  The keys of a slice are sorted by (position, symbol), so the counters a run of keys adds to lie in a narrow
/// window behind its first key: the block counts into a window of LDS counters per filter and then adds the window to the
/// table with CONTIGUOUS atomics — 64 consecutive counters per wave instruction, the shape the memory side takes at full
/// rate; a lane per scattered counter, as the first version did, is an order of magnitude slower per add (MI355X guide,
/// "Global float atomics": access shape).  The block's share of keys is cut into chunks where the window is full: as many
/// granules as end within WINDOW counters of the chunk's first (the granules' base counters tell) — thousands of keys per
/// chunk where a position has many, one granule where private substitutions lie thirteen to a position; the window is
/// flushed and reused chunk by chunk, the filter slices stay.  Lanes whose keys share a counter add through the stretch's last
/// lane only (identical addresses do not combine for LDS atomics), and the loop body has no per-key branch (see there).  No
/// barrier between a chunk's granules: the waves run on by themselves, one waits for its keys while another counts; two
/// blocks per CU for one and two filters (<= 64 VGPRs, 64 KiB of LDS) cover each other's first and last steps.  Eight filters:
/// the slices as one byte per row and the lanes' sums in packed fields (see there), one block per CU.
constexpr uint32_t ESCAPE_GRANULES_PER_BLOCK = 64;  // of a block's share, at most
template <int FILTERS>
constexpr uint32_t escapeWindow() {  // LDS counters per filter: 48 KiB of them for 1-4 filters, 28 KiB for 8 (beside 128 KiB of filter slices)
   return FILTERS >= 8 ? 896u : 12288u / FILTERS;
}
template <int FILTERS>
constexpr uint32_t escapeLdsBytes() {
   return (FILTERS * (ESCAPE_SLICE_WORDS32 + escapeWindow<FILTERS>()) + 3u * ESCAPE_GRANULES_PER_BLOCK + 4u + 64u) * static_cast<uint32_t>(sizeof(uint32_t));
}

/// What a block keeps in LDS from one item to the next (both uniform).
struct EscapeBlockState {
   uint32_t slice;  // the slice whose filters are in LDS; ~0: none yet
   bool any_row;    // ... and whether any of its rows is selected by a filter of the pass
   bool zeroed;     // the counter windows have been zeroed: by the block's first item that gets as far as its filter slices
};

/// One ITEM of k_scan_escapes_sliced (see there): the share `item` numbers — (range, slice, share) — counted by the whole block.
/// Every `return` is taken by all 16 waves, and a barrier lies between the last read of an item's list of granules or of the
/// filter slices and the next item's rewrite of them: the last one of flushChunk, the one behind the filter slices, or the one
/// of the exit without a live granule.  The counter windows are zeroed ONCE per block, by its first item that gets past the exits
/// without keys or live granules (a block that only finds such items never pays for it): flushChunk leaves every counter it
/// flushed at zero, and an item that leaves early has not touched them.
/// WALK = false: the block has this one item — nothing is kept, no exit needs a barrier, and the code is that of a kernel
/// without items (the launch of one block per item, the default, pays nothing for the walk).
template <int FILTERS, bool WALK>
__device__ __forceinline__ void scanEscapeItem(const EscapeSliceArgs& args, const uint32_t n_filters, const uint32_t item, EscapeBlockState& kept) {
   constexpr uint32_t WINDOW = escapeWindow<FILTERS>();
   static_assert(ESCAPE_GRANULE_KEYS == ESCAPE_SLICE_THREADS * 4u, "a granule is one 16-byte load per thread of the block");
   extern __shared__ uint32_t s_filter[];  // [FILTERS][ESCAPE_SLICE_WORDS32], then the counters [FILTERS][WINDOW], the granules' bases, the chunks' last keys
   uint32_t* s_count = s_filter + FILTERS * ESCAPE_SLICE_WORDS32;
   // the LIVE granules of the share — all of them, or those a pruning scan does not skip —, in order: the counter of each one's
   // first key, one past the counter of its last key (the next granule's first; for the share's last granule one past its last
   // key's), its number within the share; s_live[ESCAPE_GRANULES_PER_BLOCK] = how many there are
   uint32_t* s_base = s_count + FILTERS * WINDOW;           // [ESCAPE_GRANULES_PER_BLOCK]
   uint32_t* s_end = s_base + ESCAPE_GRANULES_PER_BLOCK;    // [ESCAPE_GRANULES_PER_BLOCK]
   uint32_t* s_live = s_end + ESCAPE_GRANULES_PER_BLOCK;    // [ESCAPE_GRANULES_PER_BLOCK + 1]
   uint32_t* s_nowhere = s_live + ESCAPE_GRANULES_PER_BLOCK + 4u;  // [64] a word per lane: where an add of nothing goes
   const uint32_t first_filter = blockIdx.z * FILTERS;
   uint32_t r = 0;
   while (r + 1u < args.n_ranges && item >= args.ranges[r + 1u].first_item) {  // (uniform)
      ++r;
   }
   const EscapeSliceArgs::Range& range = args.ranges[r];
   const uint32_t slice = (item - range.first_item) / range.items_per_slice;
   const uint32_t share = (item - range.first_item) % range.items_per_slice;
   const uint32_t out_symbols = range.out_symbols;
   const uint32_t* first = range.slice_first + static_cast<size_t>(slice) * (range.positions + 1u);
   const uint32_t key_begin = first[range.key_from];
   const uint32_t key_end = first[range.pos_end];
   // the item's share: args.block_keys keys (whole granules)
   const uint32_t share_begin = key_begin / ESCAPE_GRANULE_KEYS * ESCAPE_GRANULE_KEYS + share * args.block_keys;
   if (share_begin >= key_end) {
      return;  // (uniform) no keys for this item
   }
   // the filter slices stay in LDS while the block's items stay in one slice; a slice none of whose rows is selected is left at once
   const bool reload = !WALK || slice != kept.slice;  // (uniform)
   if (!reload && !kept.any_row) {
      return;
   }
   const uint32_t share_end = min(share_begin + args.block_keys, key_end);
   const uint32_t range_first = range.pos_begin * out_symbols;
   const bool clamp = range.key_from < range.pos_begin;  // (uniform) gap events before the range's first position
   // Everything the block reads first is asked for at once, behind the one dependent load of the slice index: the filter
   // slices, the first keys, the granules' base counters, the share's last key — every memory latency put in a row would
   // show; the keys of the granule after the next are asked for while a granule is counted, across the chunks.
   const uint32_t first_granule = share_begin / ESCAPE_GRANULE_KEYS;
   const uint32_t n_granules = (share_end - share_begin + ESCAPE_GRANULE_KEYS - 1u) / ESCAPE_GRANULE_KEYS;  // <= ESCAPE_GRANULES_PER_BLOCK
   // (unconditional: a load under a condition, or a loaded register handed on by a move, makes the compiler wait for ALL loads
   // in flight where the first is used — vmcnt(0) in the loop took a memory latency per granule: 86 us for 73 M keys.  A granule
   // past the share's last reads that one again; the whole granule exists, padded, past the slice's last key.)
   const auto loadGranule = [&](uint32_t granule) {  // (its number within the share)
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(range.keys + share_begin + granule * ESCAPE_GRANULE_KEYS + threadIdx.x * 4u));
      return make_uint4(v.x, v.y, v.z, v.w);
   };
   // The list of live granules, by the block's first wave (a share has at most 64 granules: one per lane).  A pruning scan
   // skips a granule where NO filter of the pass can report a row from its keys (granulePrunable: the select kernel's own
   // arithmetic on a lower bound of the rows covered); the counts of such keys end up on the position's derived symbol.
   const bool prune = range.heaviest != nullptr;  // (uniform)
   const auto listGranules = [&]() {
      if (threadIdx.x >= 64u) {
         return;
      }
      const bool in_share = threadIdx.x < n_granules;
      bool live = in_share;
      if (prune && in_share) {
         const uint32_t heaviest = range.heaviest[first_granule + threadIdx.x];
         const uint32_t without = range.without[first_granule + threadIdx.x];
         bool skip = true;
#pragma unroll
         for (int f = 0; f < FILTERS; ++f) {
            if (first_filter + f < n_filters) {
               skip = skip && granulePrunable(args.counters[(first_filter + f) * SPARSE_COUNTER_STRIDE + 2u], without, heaviest, args.min_proportion[first_filter + f]);
            }
         }
         live = !skip;
      }
      const uint64_t live_lanes = __ballot(live);
      if (live) {
         const uint32_t k = static_cast<uint32_t>(__popcll(live_lanes & ((uint64_t{1} << threadIdx.x) - 1u)));
         s_live[k] = threadIdx.x;
         s_base[k] = range.granule_base[first_granule + threadIdx.x];
         // (a key that went to the overflow list reads as the largest relative counter: a wider window, nothing else)
         s_end[k] = threadIdx.x + 1u < n_granules ? range.granule_base[first_granule + threadIdx.x + 1u]
                                                  : range.granule_base[first_granule + threadIdx.x] + (range.keys[share_end - 1u] >> ESCAPE_SLICE_SHIFT) + 1u;
      }
      if (threadIdx.x == 0) {
         s_live[ESCAPE_GRANULES_PER_BLOCK] = static_cast<uint32_t>(__popcll(live_lanes));
      }
   };
   // (the list's entries are the same for every lane: kept in scalar registers, not one vector register each)
   const auto liveGranule = [&](uint32_t k) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_live[k]))); };
   uint32_t n_live = n_granules;
   if (prune) {  // (uniform) the list first: a block whose granules all skip leaves before it asks for its filter slices and keys
      listGranules();
      __syncthreads();
      n_live = liveGranule(ESCAPE_GRANULES_PER_BLOCK);
      if (n_live == 0) {
         if constexpr (WALK) {
            ldsBarrier();  // (every wave has read the count before the next item's list overwrites it)
         }
         return;
      }
   }
   const auto loadKeys = [&](uint32_t k) {  // the k-th live granule; past the last: that one again
      return loadGranule(liveGranule(min(k, n_live - 1u)));
   };
   uint64_t any_bit = 0;
   ulonglong2 filter_part[FILTERS][ESCAPE_SLICE_WORDS32 / 4u / ESCAPE_SLICE_THREADS];
#pragma unroll
   for (int f = 0; f < FILTERS; ++f) {  // this slice of every filter, unless LDS has it: 16 bytes per thread, zeros past the end of the row (and for a filter past the last)
      const uint32_t first_word = slice * (ESCAPE_SLICE_WORDS32 / 2u);
      const bool present = first_filter + f < n_filters;
      const uint64_t* filter = args.filters[present ? first_filter + f : first_filter];
#pragma unroll
      for (uint32_t j = 0; j < ESCAPE_SLICE_WORDS32 / 4u / ESCAPE_SLICE_THREADS; ++j) {
         const uint32_t word = first_word + (j * ESCAPE_SLICE_THREADS + threadIdx.x) * 2u;  // 16-byte chunk of the slice
         filter_part[f][j] = reload && present && word < args.row_words ? *reinterpret_cast<const ulonglong2*>(filter + word) : make_ulonglong2(0, 0);
      }
   }
   // three granules in flight per wave, in registers of their own (without pruning the list is not written yet: granule k is live granule k)
   uint4 quad0 = prune ? loadKeys(0) : loadGranule(0);
   uint4 quad1 = prune ? loadKeys(1) : loadGranule(min(1u, n_granules - 1u));
   uint4 quad2 = prune ? loadKeys(2) : loadGranule(min(2u, n_granules - 1u));
   if (!prune) {
      listGranules();
   }
   // Eight filters: their slices are kept as ONE BYTE PER ROW — bit f = filter f has the row — so that a key's lookup is one
   // LDS read for all eight (a read per filter and key made the eight-filter pass LDS-bound: 32 of its ~70 LDS instructions
   // per granule and wave).  A thread holds the 128 rows of its 16-byte part of every filter and writes their 128 bytes.
   constexpr bool BYTE_PER_ROW = FILTERS == 8;
   static_assert(ESCAPE_SLICE_WORDS32 / 4u / ESCAPE_SLICE_THREADS == 1u, "a thread holds one 16-byte part of a filter slice");
   if (!WALK || !kept.zeroed) {  // (uniform; the barrier below stands between these stores and the first add)
      for (uint32_t j = threadIdx.x * 4u; j < FILTERS * WINDOW; j += ESCAPE_SLICE_THREADS * 4u) {  // (16 bytes per store; WINDOW is a multiple of 4)
         *reinterpret_cast<uint4*>(s_count + j) = make_uint4(0, 0, 0, 0);
      }
      kept.zeroed = true;
   }
   if (!reload) {
      ldsBarrier();  // (the list of granules, where the first wave has just written it)
   } else {
#pragma unroll
      for (int f = 0; f < FILTERS; ++f) {
         if constexpr (!BYTE_PER_ROW) {
            *reinterpret_cast<ulonglong2*>(s_filter + f * ESCAPE_SLICE_WORDS32 + threadIdx.x * 4u) = filter_part[f][0];
         }
         any_bit |= filter_part[f][0].x | filter_part[f][0].y;
      }
      if constexpr (BYTE_PER_ROW) {
#pragma unroll
         for (uint32_t quarter = 0; quarter < 4; ++quarter) {  // 32 rows of the thread's 128: 32 bytes
            uint32_t bytes[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
               bytes[k] = 0;
            }
#pragma unroll
            for (int f = 0; f < FILTERS; ++f) {
               const uint64_t half = quarter < 2 ? filter_part[f][0].x : filter_part[f][0].y;
               const uint32_t rows32 = static_cast<uint32_t>(half >> (32u * (quarter & 1u)));
#pragma unroll
               for (uint32_t k = 0; k < 8; ++k) {  // four rows -> the low bits of four bytes
                  bytes[k] |= ((((rows32 >> (4u * k)) & 0xFu) * 0x00204081u) & 0x01010101u) << f;
               }
            }
            uint32_t* out = s_filter + threadIdx.x * 32u + quarter * 8u;  // (row r of the slice = byte r)
            *reinterpret_cast<uint4*>(out) = make_uint4(bytes[0], bytes[1], bytes[2], bytes[3]);
            *reinterpret_cast<uint4*>(out + 4) = make_uint4(bytes[4], bytes[5], bytes[6], bytes[7]);
         }
      }
      kept.any_row = __syncthreads_or(any_bit != 0 ? 1 : 0) != 0;
      kept.slice = slice;
   }
   if (!kept.any_row) {
      return;  // no row of this slice is selected: none of its keys counts
   }
   const uint32_t lane = __lane_id();
   // the chunk being counted: the granules up to chunk_granules, its window of counters
   uint32_t window_first = 0, window_used = 0, chunk_granules = 0, chunk_end = 0;
   const auto beginChunk = [&](uint32_t g) {
      // the window begins at the chunk's first key's position (the range's first position where the granule begins before it)
      // and takes the granules that end within WINDOW counters of that, one at least
      const uint32_t first_counter = max(s_base[g], range_first);
      window_first = first_counter / out_symbols * out_symbols - range_first;
      uint32_t h = g + 1u;
      while (h < n_live && max(s_end[h], range_first) - range_first - window_first < WINDOW) {  // (a granule's last key may sit on the next one's first counter)
         ++h;
      }
      chunk_granules = h;
      chunk_end = min(share_begin + (liveGranule(h - 1u) + 1u) * ESCAPE_GRANULE_KEYS, share_end);
      window_used = min(WINDOW, (max(s_end[h - 1u], range_first) / out_symbols + 1u) * out_symbols - range_first - window_first);
   };
   // the chunk's window goes to the table — contiguous atomics, 64 consecutive counters per wave instruction — and is zero
   // again for the next chunk
   const auto flushChunk = [&]() {
      ldsBarrier();
#pragma unroll
      for (int f = 0; f < FILTERS; ++f) {
         uint32_t* __restrict__ counts = range.counts[first_filter + f < n_filters ? first_filter + f : first_filter] + window_first;
         for (uint32_t j = threadIdx.x; j < window_used; j += ESCAPE_SLICE_THREADS) {
            const uint32_t value = s_count[f * WINDOW + j];
            if (value != 0) {
               s_count[f * WINDOW + j] = 0;
               atomicAdd(&counts[j], value);
            }
         }
      }
      ldsBarrier();
   };
   const auto countGranule = [&](uint4& in_flight, uint32_t g) {  // (g is uniform: the g-th live granule)
      if (g >= n_live) {
         return;
      }
      if (g == chunk_granules) {
         flushChunk();
         beginChunk(g);
      }
      const uint4 quad = in_flight;
      in_flight = loadKeys(g + 3u);
      const uint32_t granule_first = share_begin + liveGranule(g) * ESCAPE_GRANULE_KEYS;
      {
         const uint32_t granule_counter = s_base[g] - range_first - window_first;  // (wraps below the window: such keys are masked)
         const uint32_t i = granule_first + threadIdx.x * 4u;
         const uint32_t keys4[4] = {quad.x, quad.y, quad.z, quad.w};
         uint32_t in_window[4];
         bool valid[4];
         // the keys before the scanned positions' first and behind their last, read along in the first and the last granule, are masked out
         // (one unsigned comparison per key: index - first valid index < number of valid indices)
         if (granule_first >= key_begin && granule_first + ESCAPE_GRANULE_KEYS <= chunk_end) {  // (uniform) the granule lies inside: nearly all do
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
               valid[c] = keys4[c] != ESCAPE_KEY_INVALID;
            }
         } else {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
               valid[c] = static_cast<bool>(static_cast<uint32_t>(keys4[c] != ESCAPE_KEY_INVALID) & static_cast<uint32_t>(i + c - key_begin < chunk_end - key_begin));
            }
         }
#pragma unroll
         for (uint32_t c = 0; c < 4; ++c) {
            in_window[c] = granule_counter + (keys4[c] >> ESCAPE_SLICE_SHIFT);
         }
         if (clamp && s_base[g] < range_first) {  // (uniform) a gap event before the range's first position counts on its counters:
            // the window begins there (window_first = 0) and an event below it keeps its kind (range_first is even)
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
               in_window[c] = static_cast<int32_t>(in_window[c]) < 0 ? in_window[c] & 1u : in_window[c];
            }
         }
         // A lane's four keys are consecutive keys of the sorted list.  Those on the counter of its first key are summed in the
         // lane (n0 <= 4); across the lanes these first counters ascend, lanes on the same one form a stretch, and a stretch adds
         // ONCE, through its last lane: the selected keys of the lanes up to and including it (population counts of the wave's
         // ballots of the bits of n0) minus those before the stretch's first lane (fetched from that lane) — no 64 lanes on one
         // LDS counter (identical addresses do not combine: ~12 cycles per lane), no add at all for a stretch without a selected
         // key (the keys read along outside the chunk lie in such stretches), and ~80 instructions per four keys where a stretch
         // mask per key column took 300.  A key on another counter than the lane's first (a lane on a boundary) adds by itself.
         const uint32_t counter0 = in_window[0];
         const uint32_t previous = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(counter0), 0x138 /* wave_shr:1 */, 0xF, 0xF, false));
         const uint32_t following = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(counter0), 0x130 /* wave_shl:1 */, 0xF, 0xF, false));
         const bool head = lane == 0 || counter0 != previous;
         const bool tail = lane == 63 || counter0 != following;
         const uint64_t heads_at_or_below = __ballot(head) & (~uint64_t{0} >> (63u - lane));  // (lane 0 is one: never empty)
         const uint32_t first_of_stretch = 63u - static_cast<uint32_t>(__builtin_clzll(heads_at_or_below));
         // The body has no per-key branch: an add that has nothing to add goes to a word of the lane's own (64 lanes adding zero
         // to one counter would still serialise) — 4 LDS atomics per granule and filter whatever the keys.  Where a granule by
         // itself always fits the window (FILTERS <= 2: ESCAPE_MAX_RELATIVE) every selected key of a chunk lies inside it and
         // there is no second path either.  With per-key branches and a table path through a merged (flat) address the body
         // took 250 instructions per granule and wave, half of them exec-mask traffic, and the kernel was bound by them
         // (profiles/r03_notes.md): 151 now.
         constexpr bool EVERY_KEY_IN_WINDOW = WINDOW >= ESCAPE_MAX_RELATIVE + 64u;
         [[maybe_unused]] uint32_t filters_with[4] = {0, 0, 0, 0};  // (one byte per row: bit f = filter f has the key's row)
         if constexpr (BYTE_PER_ROW) {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
               filters_with[c] = reinterpret_cast<const uint8_t*>(s_filter)[keys4[c] & ESCAPE_ROW_MASK] & (valid[c] ? 0xFFu : 0u);  // (the read itself is always inside the slice)
            }
         }
         if constexpr (BYTE_PER_ROW) {
            // Eight filters at once.  The lane's sums per filter (<= 4) sit two to a register in 16-bit fields, so ONE inclusive
            // scan over the lanes (6 DPP adds per register) gives every filter's prefix, and one ds_bpermute per register the
            // prefixes at the stretch's first lane; only the final adds are per filter.  (Filter by filter — ballots, mbcnt,
            // a bpermute each — the pass cost eight times the one-filter kernel per key: 2/3 of the configs[4] batch.)
            const auto add8 = [&](uint32_t counter, uint32_t value, int f) {
               const bool here = value != 0 && counter < WINDOW;
               if (__ballot(here) != 0) {
                  atomicAdd(here ? &s_count[f * WINDOW + counter] : &s_nowhere[lane], here ? value : 0u);
               }
               if (value != 0 && counter >= WINDOW) {  // a key past the window: straight to the table
                  atomicAdd(&range.counts[first_filter + f < n_filters ? first_filter + f : first_filter][window_first + counter], value);
               }
            };
            uint32_t on_first = filters_with[0];          // per key: the filters that have it, if it sits on the lane's first counter
            uint32_t sums[4] = {0, 0, 0, 0};              // [k]: filters 2k (low field) and 2k + 1 (high field)
            uint32_t elsewhere[4] = {0, 0, 0, 0};         // per key: the filters that have it, if it sits on another counter
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
               if (c != 0) {
                  const bool same = in_window[c] == counter0;
                  on_first = same ? filters_with[c] : 0u;
                  elsewhere[c] = same ? 0u : filters_with[c];
               }
#pragma unroll
               for (uint32_t k = 0; k < 4; ++k) {
                  sums[k] += ((on_first >> (2u * k)) & 1u) | (((on_first >> (2u * k + 1u)) & 1u) << 16);
               }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
               const uint32_t through = waveSumToLane63(sums[k]);  // (inclusive scan over the lanes: <= 256 per field)
               const uint32_t before = through - sums[k];
               const uint32_t before_stretch = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(static_cast<int>(first_of_stretch * 4u), static_cast<int>(before)));
               const uint32_t stretch = through - before_stretch;  // (field by field: no borrow, a prefix never exceeds a later one)
               add8(counter0, tail ? stretch & 0xFFFFu : 0u, static_cast<int>(2u * k));
               add8(counter0, tail ? stretch >> 16 : 0u, static_cast<int>(2u * k + 1u));
            }
#pragma unroll
            for (uint32_t c = 1; c < 4; ++c) {
               if (__ballot(elsewhere[c] != 0) != 0) {  // (uniform) a lane on a boundary of counters
#pragma unroll
                  for (int f = 0; f < FILTERS; ++f) {
                     add8(in_window[c], (elsewhere[c] >> f) & 1u, f);
                  }
               }
            }
            return;
         }
#pragma unroll
         for (int f = 0; f < FILTERS; ++f) {
            uint32_t* __restrict__ window = s_count + f * WINDOW;
            // (an add of nothing goes to the lane's own word; where a key may lie past the window it goes to the table by itself)
            [[maybe_unused]] uint32_t* __restrict__ table = range.counts[first_filter + f < n_filters ? first_filter + f : first_filter] + window_first;
            const auto add = [&](uint32_t counter, uint32_t value) {
               const bool here = EVERY_KEY_IN_WINDOW ? value != 0 : value != 0 && counter < WINDOW;
               atomicAdd(here ? &window[counter] : &s_nowhere[lane], here ? value : 0u);
               if constexpr (!EVERY_KEY_IN_WINDOW) {
                  if (value != 0 && counter >= WINDOW) {
                     atomicAdd(&table[counter], value);
                  }
               }
            };
            uint32_t n0 = 0;
            uint32_t elsewhere[4] = {0, 0, 0, 0};  // a key of the lane on another counter than its first, selected
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
               const uint32_t row = keys4[c] & ESCAPE_ROW_MASK;
               const uint32_t selected = (s_filter[f * ESCAPE_SLICE_WORDS32 + (row >> 5)] >> (row & 31u)) & (valid[c] ? 1u : 0u);  // (the read itself is always inside the slice)
               if (c == 0) {
                  n0 = selected;
               } else {
                  const bool same = in_window[c] == counter0;
                  n0 += same ? selected : 0u;
                  elsewhere[c] = same ? 0u : selected;
               }
            }
            if (__ballot((elsewhere[1] | elsewhere[2] | elsewhere[3]) != 0) != 0) {  // (uniform: where the keys are many to a counter no lane has one)
#pragma unroll
               for (uint32_t c = 1; c < 4; ++c) {
                  add(in_window[c], elsewhere[c]);
               }
            }
            // the stretch's sum at its last lane: an inclusive scan of the lanes' sums (6 DPP adds) less the prefix at its first lane
            const uint32_t through = waveSumToLane63(n0);
            const uint32_t before_stretch = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(static_cast<int>(first_of_stretch * 4u), static_cast<int>(through - n0)));
            add(counter0, tail ? through - before_stretch : 0u);
         }
      }
   };
   beginChunk(0);
   for (uint32_t g = 0; g < n_live; g += 3u) {  // (uniform)
      countGranule(quad0, g);
      countGranule(quad1, g + 1u);
      countGranule(quad2, g + 2u);
   }
   flushChunk();
}

/// WALK: the blocks of the launch walk its items in turn — block b takes the items b, b + gridDim.x, ... below args.n_items; any
/// number of blocks gives the same tables, and nothing passes between blocks but the adds to the tables.  !WALK: gridDim.x =
/// args.n_items, block b counts item b.  The host chooses (escape_item_plan.h, SILO_GPU_TUNE_ESCAPE_BLOCKS): one block per
/// item by default — measured, the chip's own dealing of more blocks than it holds evens out the items better than a strided
/// deal to resident blocks saves in block starts (profiles/r10_escape_items.md).
/// (Registers: one and two filters run two blocks to a CU and stay within 64 VGPRs; four and eight filters fill the LDS of a CU
/// with one block, 4 waves per SIMD; the walk of four filters needs more than 64 VGPRs for what it keeps and may take 128.)
template <int FILTERS, bool WALK>
__global__ __launch_bounds__(ESCAPE_SLICE_THREADS, (FILTERS <= 2 || (FILTERS <= 4 && !WALK)) ? 8 : 4) void k_scan_escapes_sliced(const EscapeSliceArgs args, uint32_t n_filters) {
   EscapeBlockState kept{~0u, false, false};
   if constexpr (!WALK) {
      scanEscapeItem<FILTERS, false>(args, n_filters, blockIdx.x, kept);
   } else {
      for (uint32_t item = blockIdx.x; item < args.n_items; item += gridDim.x) {  // (uniform; n_items + gridDim.x does not wrap: ESCAPE_PLAN_MAX_ITEMS)
         scanEscapeItem<FILTERS, true>(args, n_filters, item, kept);
      }
   }
}

/// The few keys of a store that do not fit the packed form (SliceMajorKeys::d_overflow of SeqStoreHost::Layout::escapes_sliced: counter << 32 | sequence),
/// for the positions [pos_begin, pos_end): one global filter lookup and one atomic each; grid.y = filter.
__global__ __launch_bounds__(256) void k_scan_escapes_overflow(
   const uint64_t* __restrict__ keys, uint32_t n_keys, const ScanBatchArgs batch, uint32_t pos_begin, uint32_t pos_end
) {
   const uint32_t q = blockIdx.y;
   const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n_keys) {
      return;
   }
   const uint64_t key = keys[i];
   const uint32_t counter = static_cast<uint32_t>(key >> 32);
   const uint32_t sequence = static_cast<uint32_t>(key);
   if (counter >= pos_begin * batch.out_symbols && counter < pos_end * batch.out_symbols && ((batch.filters[q][sequence >> 6] >> (sequence & 63u)) & 1ull) != 0) {
      atomicAdd(&batch.counts[0][q][counter - pos_begin * batch.out_symbols], 1u);
   }
}

static_assert(ESCAPE_PLAN_MAX_ENTRIES == ESCAPE_MAX_RANGES && ESCAPE_PLAN_GRANULE_KEYS == ESCAPE_GRANULE_KEYS && ESCAPE_PLAN_GRANULES_PER_ITEM == ESCAPE_GRANULES_PER_BLOCK,
   "escape_item_plan.h repeats these constants so that it needs no HIP");

/// k_scan_escapes_sliced<FILTERS, WALK>: what a launch needs of an instantiation.
template <int FILTERS, bool WALK>
void launchEscapes(const dim3 grid, hipStream_t stream, const EscapeSliceArgs& args, uint32_t n_filters) {
   k_scan_escapes_sliced<FILTERS, WALK><<<grid, ESCAPE_SLICE_THREADS, escapeLdsBytes<FILTERS>(), stream>>>(args, n_filters);
}
template <int FILTERS, bool WALK>
hipError_t prepareEscapes(int* blocks_per_cu) {  // more dynamic LDS than a kernel may ask for by default; its resident blocks per CU
   if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_scan_escapes_sliced<FILTERS, WALK>), hipFuncAttributeMaxDynamicSharedMemorySize, escapeLdsBytes<FILTERS>());
       e != hipSuccess) {
      return e;
   }
   return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_scan_escapes_sliced<FILTERS, WALK>, ESCAPE_SLICE_THREADS, escapeLdsBytes<FILTERS>());
}
template <bool WALK>
void launchEscapes(uint32_t per_block, const dim3 grid, hipStream_t stream, const EscapeSliceArgs& args, uint32_t n_filters) {
   switch (per_block) {
      case 1: launchEscapes<1, WALK>(grid, stream, args, n_filters); break;
      case 2: launchEscapes<2, WALK>(grid, stream, args, n_filters); break;
      case 4: launchEscapes<4, WALK>(grid, stream, args, n_filters); break;
      default: launchEscapes<8, WALK>(grid, stream, args, n_filters); break;
   }
}
template <bool WALK>
hipError_t prepareEscapes(uint32_t per_block, int* blocks_per_cu) {
   switch (per_block) {
      case 1: return prepareEscapes<1, WALK>(blocks_per_cu);
      case 2: return prepareEscapes<2, WALK>(blocks_per_cu);
      case 4: return prepareEscapes<4, WALK>(blocks_per_cu);
      default: return prepareEscapes<8, WALK>(blocks_per_cu);
   }
}

/// Blocks of k_scan_escapes_sliced<per_block, walk> that the current device holds at once: resident blocks per CU (the occupancy
/// query, with the kernel's LDS) x CUs.  Asked once per device and instantiation, with the kernel's LDS attribute set in the same
/// step; afterwards one relaxed load (two threads that ask at once both ask the runtime and store the same answer).
hipError_t escapePlaces(uint32_t per_block, bool walk, uint32_t* out) {
   constexpr int MAX_DEVICES = 64;
   static std::atomic<uint32_t> cached[MAX_DEVICES][4][2];
   int device = 0;
   if (const hipError_t e = hipGetDevice(&device); e != hipSuccess) {
      return e;
   }
   if (device < 0 || device >= MAX_DEVICES) {
      return hipErrorInvalidDevice;
   }
   std::atomic<uint32_t>& slot = cached[device][per_block == 1 ? 0 : (per_block == 2 ? 1 : (per_block == 4 ? 2 : 3))][walk ? 1 : 0];
   *out = slot.load(std::memory_order_relaxed);
   if (*out != 0) {
      return hipSuccess;
   }
   int per_cu = 0, cus = 0;
   if (const hipError_t e = walk ? prepareEscapes<true>(per_block, &per_cu) : prepareEscapes<false>(per_block, &per_cu); e != hipSuccess) {
      return e;
   }
   if (const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device); e != hipSuccess) {
      return e;
   }
   *out = static_cast<uint32_t>(std::max(1, per_cu)) * static_cast<uint32_t>(std::max(1, cus));
   slot.store(*out, std::memory_order_relaxed);
   return hipSuccess;
}

/// The launch descriptor of the position-major and the overflow keys of `range`: its filters and its count tables.
ScanBatchArgs keyBatch(const ScanRange& range, const uint64_t* const* filters, uint32_t q_count) {
   ScanBatchArgs batch{};
   batch.out_symbols = range.seqstore->dev.n_scan;
   copyFilters(batch.filters, filters, q_count);
   std::copy_n(range.counts, q_count, batch.counts[0]);
   return batch;
}

}  // namespace

namespace silo_gpu_detail {

thread_local uint32_t g_last_escape_items = 0;

/// The rows the code planes do not carry: one pass over the escape keys of every range, for all filters (dense and
/// sparse alike: the gather reads the same planes); with `gaps` (one entry per range: its store and positions, counts = the range's gap tables,
/// null where it has none) also the gap events of their stores, in the same launches.
/// With `gaps` and pruning->keys the pass may skip the granules of keys that no Mutations row of the filters' proportions can come
/// from, where the store has the bounds for it (EscapeSliceArgs::counters); the gap events and the overflow keys are always counted.
/// With `ends` (one entry per range: counts = the range's ends tables, seqstore null where the range reads its rows) two more
/// entries per such range in the same launches: the end events of the gap symbol, counted like gap events, and the residual keys
/// of the covered rows, counted into the range's count tables like escape keys; neither is ever skipped.  only_ends: nothing but
/// these entries (SILO_GPU_TUNE_END_RUNS = 1: the end events in a launch of their own, for comparisons).
int scanEscapes(
   const std::vector<ScanRange>& ranges, const uint64_t* const* filters, uint32_t q_count, hipStream_t hip_stream, const std::vector<ScanRange>* gaps,
   const ScanPruning* pruning, const std::vector<ScanRange>* ends, bool only_ends
) {
   // the ranges whose stores have slice-major keys go ESCAPE_MAX_RANGES at a time into one launch of k_scan_escapes_sliced
   EscapeSliceArgs sliced{};
   copyFilters(sliced.filters, filters, q_count);
   const bool prune = gaps != nullptr && pruning != nullptr && pruning->keys;
   if (prune) {
      std::copy_n(pruning->min_proportion, q_count, sliced.min_proportion);
      sliced.counters = pruning->counters;
   }
   uint32_t n_sliced = 0;
   std::array<EscapeEntryShape, ESCAPE_MAX_RANGES> shapes{};  // most_keys: of one (range, slice)
   uint64_t total_keys = 0;  // of the ranges of the launch
   bool end_entries = false;  // the launch has end events or residual keys (", ends" behind the kernel's name in the timing log)
   const auto launchSliced = [&]() -> int {
      if (n_sliced == 0) {
         return SILO_GPU_OK;
      }
      const uint32_t per_block = q_count <= 1 ? 1 : (q_count <= 2 ? 2 : (q_count <= 4 ? 4 : 8));  // filters per pass over the keys
      const uint32_t passes = (q_count + per_block - 1) / per_block;
      // The items of the launch — every range as many per slice as its slice with the most keys needs, the never-pruned ranges
      // first —, their size and the blocks that walk them: escape_item_plan.h.  The ranges go to the kernel in the items' order.
      const int knob = g_tune_escape_blocks.load();
      uint32_t places = 0, walk_places = 0;
      HIP_TRY(escapePlaces(per_block, false, &places));
      if (knob != 0) {  // (the walking instantiation: its own attribute, and its own places where the knob asks for resident blocks)
         HIP_TRY(escapePlaces(per_block, true, knob < 0 ? &places : &walk_places));
      }
      const EscapeItemPlan plan = planEscapeItems(shapes.data(), n_sliced, sliced.n_slices, passes, places, knob);
      if (!plan.ok) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "scanEscapes: the launch has more items than the escape kernel numbers");
      }
      sliced.block_keys = plan.block_keys;
      sliced.n_ranges = n_sliced;
      sliced.n_items = plan.n_items;
      std::array<EscapeSliceArgs::Range, ESCAPE_MAX_RANGES> as_added{};
      std::copy_n(sliced.ranges, n_sliced, as_added.begin());
      for (uint32_t k = 0; k < n_sliced; ++k) {
         sliced.ranges[k] = as_added[plan.order[k]];
         sliced.ranges[k].first_item = plan.first_item[k];
         sliced.ranges[k].items_per_slice = plan.items_per_slice[k];
      }
      g_last_escape_items = plan.n_items;
      const dim3 grid(plan.grid, 1, passes);
      char name[64];
      bool bounds = false;  // a launch that may skip granules says so in the timing log (", pruning" behind the kernel's name)
      for (uint32_t k = 0; k < n_sliced; ++k) {
         bounds = bounds || sliced.ranges[k].heaviest != nullptr;
      }
      std::snprintf(name, sizeof(name), "k_scan_escapes_sliced<%u>%s%s", per_block, bounds ? ", pruning" : "", end_entries ? ", ends" : "");
      // bytes: the keys and gap events (4 each) once per pass of `per_block` filters, plus a 16 KiB filter slice per ITEM and filter
      // (what one block per item reads: the figure stays comparable whatever the grid); blocks: the grid as launched
      ScanLaunchTiming* timing = startLaunchTiming(
         name, 0, total_keys * sizeof(uint32_t) * grid.z + static_cast<uint64_t>(plan.n_items) * q_count * ESCAPE_SLICE_WORDS32 * sizeof(uint32_t), q_count,
         grid.x * grid.z, hip_stream
      );
      if (plan.grid < plan.n_items) {
         launchEscapes<true>(per_block, grid, hip_stream, sliced, q_count);
      } else {
         launchEscapes<false>(per_block, grid, hip_stream, sliced, q_count);
      }
      HIP_TRY(hipGetLastError());
      finishLaunchTiming(timing, hip_stream);
      n_sliced = 0;
      shapes.fill(EscapeEntryShape{});
      total_keys = 0;
      end_entries = false;
      return SILO_GPU_OK;
   };
   // one entry of a launch: the packed keys (or gap events) of a store over [key_from, pos_end) of its positions
   const auto addSliced = [&](const ScanRange& range, const SliceMajorKeys& stream, uint32_t out_symbols, uint32_t key_from, const uint32_t* heaviest = nullptr,
                              const uint32_t* without = nullptr) -> int {
      const uint32_t n_slices = stream.n_slices;
      if (n_sliced == ESCAPE_MAX_RANGES || (n_sliced != 0 && sliced.n_slices != n_slices)) {
         if (const int rc = launchSliced(); rc != SILO_GPU_OK) {
            return rc;
         }
      }
      sliced.row_words = range.seqstore->dev.row_words;
      sliced.n_slices = n_slices;
      EscapeSliceArgs::Range& entry = sliced.ranges[n_sliced];
      entry.keys = stream.d_keys.get();
      entry.granule_base = stream.d_granule_base.get();
      entry.slice_first = stream.d_slice_first.get();
      entry.heaviest = heaviest;
      entry.without = without;
      entry.positions = range.seqstore->dev.positions;
      entry.pos_begin = range.pos_begin;
      entry.pos_end = range.pos_end;
      entry.out_symbols = out_symbols;
      entry.key_from = key_from;
      std::copy_n(range.counts, q_count, entry.counts);
      const size_t stride = static_cast<size_t>(entry.positions) + 1;
      for (uint32_t slice = 0; slice < n_slices; ++slice) {
         const uint32_t n = stream.slice_first[slice * stride + range.pos_end] - stream.slice_first[slice * stride + key_from];
         total_keys += n;
         shapes[n_sliced].keys += n;
         shapes[n_sliced].most_keys = std::max(shapes[n_sliced].most_keys, n + ESCAPE_GRANULE_KEYS - 1u);  // (items start at a granule boundary)
      }
      shapes[n_sliced].prunable = heaviest != nullptr;
      ++n_sliced;
      return SILO_GPU_OK;
   };
   // the gap events of a range's store, behind its keys: from its first position on where the range begins later (see EscapeSliceArgs)
   const auto addGaps = [&](size_t r) -> int {
      const SeqStoreHost::Layout& layout = ranges[r].seqstore->layout;
      if (gaps == nullptr || (*gaps)[r].seqstore == nullptr || layout.gaps.d_keys.get() == nullptr) {
         return SILO_GPU_OK;
      }
      return addSliced((*gaps)[r], layout.gaps, 2, 0);
   };
   // the end events of a range that counts the end runs of the gap symbol — from position 0 on, clamped like the gap events: a
   // leading run that ended before the range's first position has ended there — and the residual keys of its covered rows
   const auto addEnds = [&](size_t r) -> int {
      const SeqStoreHost::Layout& layout = ranges[r].seqstore->layout;
      if (ends == nullptr || (*ends)[r].seqstore == nullptr || layout.ends.d_keys.get() == nullptr) {
         return SILO_GPU_OK;
      }
      if (const int rc = addSliced((*ends)[r], layout.ends, 2, 0); rc != SILO_GPU_OK) {
         return rc;
      }
      end_entries = true;
      if (layout.residual.d_keys.get() == nullptr) {
         return SILO_GPU_OK;
      }
      const int rc = addSliced(ranges[r], layout.residual, ranges[r].seqstore->dev.n_scan, ranges[r].pos_begin);
      end_entries = true;
      return rc;
   };
   for (size_t r = 0; r < ranges.size(); ++r) {
      const ScanRange& range = ranges[r];
      const SeqStoreHost::Layout& layout = range.seqstore->layout;
      if (const int rc = addEnds(r); rc != SILO_GPU_OK) {
         return rc;
      }
      if (only_ends) {
         continue;
      }
      const uint32_t begin = layout.built && layout.d_escapes.get() != nullptr ? layout.escape_first[range.pos_begin] : 0;
      const uint32_t count = layout.built && layout.d_escapes.get() != nullptr ? layout.escape_first[range.pos_end] - begin : 0;
      if (count == 0) {
         if (const int rc = addGaps(r); rc != SILO_GPU_OK) {
            return rc;
         }
         continue;
      }
      const SliceMajorKeys& keys = layout.escapes_sliced;
      if (keys.d_keys.get() != nullptr && g_tune_side_stream.load() != 3) {  // the slice-major keys, a slice of the filter in LDS
         if (keys.n_overflow != 0) {  // the few keys that do not fit the packed form: a small launch of their own
            k_scan_escapes_overflow<<<dim3((keys.n_overflow + 255) / 256, q_count), 256, 0, hip_stream>>>(
               keys.d_overflow.get(), keys.n_overflow, keyBatch(range, filters, q_count), range.pos_begin, range.pos_end
            );
            HIP_TRY(hipGetLastError());
         }
         const bool bounds = prune && layout.d_granule_heaviest.get() != nullptr && layout.d_granule_without.get() != nullptr;
         if (const int rc = addSliced(
                range, keys, range.seqstore->dev.n_scan, range.pos_begin, bounds ? layout.d_granule_heaviest.get() : nullptr,
                bounds ? layout.d_granule_without.get() : nullptr
             );
             rc != SILO_GPU_OK) {
            return rc;
         }
         if (const int rc = addGaps(r); rc != SILO_GPU_OK) {
            return rc;
         }
         continue;
      }
      if (const int rc = addGaps(r); rc != SILO_GPU_OK) {
         return rc;
      }
      const uint32_t keys_per_block = 256 * ESCAPE_KEYS_PER_THREAD;
      k_scan_escapes<<<dim3((count + keys_per_block - 1) / keys_per_block, q_count), 256, 0, hip_stream>>>(
         layout.d_escapes.get() + begin, count, keyBatch(range, filters, q_count), range.pos_begin
      );
      HIP_TRY(hipGetLastError());
   }
   return launchSliced();
}

}  // namespace silo_gpu_detail
