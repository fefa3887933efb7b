// silo_gpu_scan_planes.hip — the plane rows of K1, the Mutations scan ("K1 design", "K1s / selective filters",
// "One-hot rows that cannot reach minProportion"): counts[q][p][s] += popcount(filter_q & plane rows of (p, s)).
//
// Kernels:
//   K1   k_scan_sliced<BITS, NSYM, WPT, Q, KIND>    the dense scan: a column tile of the filters in registers, plane rows streamed
//   K1b  k_scan_sliced_rowwave<BITS, NSYM>          one wave per position, for rows shorter than a column tile
//        k_compact_filter                           the prepare step: sectors and cardinality of every filter, scratch zeroed
//   K1s  k_scan_gather<BITS, NSYM, POSG, KIND>      only the listed sectors of the planes, under a sparse filter
// Exported (scan_internal.h): scanShortRows, prepareScan, scanPiecesDense, scanPiecesGather.
// Everything is 64-bit integer AND / OR / popcount: HBM-bound, no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <array>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "scan_internal.h"

using namespace silo_gpu_detail;

namespace {

// ------------------------------------------------------------------------------------------------
// K1: Mutations scan over the bit-sliced planes.
//
// counts[q][p][k] += popcount(filter_q & {rows whose code at position p is k + 1}) for the NSYM valid mutation symbols,
// reading BITS = ceil(log2(NSYM + 1)) planes per position (3 for nucleotides, 5 for amino acids) instead of NSYM
// one-hot planes: 0.375 instead of 0.625 bytes per position x sequence (nuc), 0.625 instead of 2.75 (aa).
//
// Grid: blockIdx.x = position_group * n_tiles + tile.  A block owns a column tile of TILE_WORDS = 256 threads * WPT
// words of the Q filters, held in registers for the whole block lifetime (registers are the first-level staging of
// the filter, LDS only carries per-wave partial counts), and streams that tile's slice of the BITS plane rows of
// `positions_per_block` consecutive positions.  Every load is a fully coalesced, non-temporal 16 B/lane access; the
// planes of position p+1 are in flight while position p is decoded (two register buffers, unconditional clamped
// loads so that s_waitcnt keeps counting).  Decoding is pure VALU: per symbol BITS and/andn per word (constant-folded
// code bits, shared sub-terms), an AND with each filter, v_bcnt; then a 6-instruction DPP wave reduction per
// (symbol, filter).  Out-of-row chunks of the ragged last tile read word 0 against zero filters.
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_WAVES = SCAN_THREADS / 64;

// positions whose partial counts sit in LDS between two flushes: ~16 KiB of LDS whatever NSYM * Q is
template <int NSYM, int Q>
constexpr int scanPositionsBatch() {
   int batch = 512 / (NSYM * Q);
   batch -= batch & 1;
   return batch < 2 ? 2 : (batch > 64 ? 64 : batch);
}

// blocks per CU the register budget has to allow: plane buffers 2 * BITS * WPT * 2 VGPRs, filters Q * WPT * 2
template <int BITS, int NSYM, int WPT, int Q>
constexpr int scanMinBlocks() {
   if (BITS == 3 && NSYM == 7 && WPT == 8) {
      return 2;  // 7 counted symbols over 8 words per thread: 3 blocks per CU would spill
   }
   return Q == 1 ? (BITS * WPT <= 12 ? 4 : (BITS * WPT <= 18 ? 4 : (BITS <= 3 && BITS * WPT <= 24 ? 3 : 2))) : (Q <= 2 && BITS <= 3 ? 4 : (Q <= 4 && BITS <= 3 ? 3 : 2));
}

template <int BITS, int NSYM, int WPT, int Q, int KIND>
__global__ __launch_bounds__(SCAN_THREADS, (scanMinBlocks<BITS, NSYM, WPT, Q>())) void k_scan_sliced(
   const ScanBatchArgs batch, const RowPruneArgs rows, uint32_t row_words, uint32_t positions_per_block, uint32_t n_tiles
) {
   constexpr int CHUNKS = WPT / 2;  // 16-byte chunks per thread and plane
   constexpr uint32_t TILE_WORDS = SCAN_THREADS * WPT;
   constexpr int POS_BATCH = scanPositionsBatch<NSYM, Q>();
   __shared__ uint32_t s_partial[2][SCAN_WAVES][POS_BATCH][NSYM * Q];
   // one-hot rows of a pruning scan: the LIVE rows of the range, ascending, and behind them how many there are
   [[maybe_unused]] __shared__ uint32_t s_live_rows[KIND == KIND_ROWS ? ROW_LIST_MAX + 1u : 1u];

   const uint32_t tid = threadIdx.x;
   const uint32_t wave = tid >> 6;
   const bool writer = (tid & 63u) == 63u;  // waveSumToLane63 leaves the total in lane 63
   uint32_t range = 0;
   while (range + 1 < batch.n_ranges && blockIdx.x >= batch.first_unit[range + 1]) {
      ++range;
   }
   const uint32_t block_in_range = blockIdx.x - batch.first_unit[range];
   const uint64_t* __restrict__ planes = batch.planes[range];
   // one-hot rows: a "position" of the pipeline is a PAIR of rows (BITS = NSYM = 2), each counted on its own
   static_assert(KIND != KIND_ROWS || (BITS == 2 && NSYM == 2), "rows are scanned in pairs");
   const uint32_t n_rows = batch.n_positions[range];
   const uint32_t n_positions = KIND == KIND_ROWS ? (n_rows + 1u) / 2u : n_rows;
   const uint32_t tile = block_in_range % n_tiles;
   const uint32_t position_group = block_in_range / n_tiles;
   uint32_t pos_begin = position_group * positions_per_block;
   uint32_t pos_end = min(n_positions, pos_begin + positions_per_block);

   // filters routed to the gather kernel count as empty here; a block with nothing left to do leaves at once
   bool dense[Q];
#pragma unroll
   for (int q = 0; q < Q; ++q) {
      dense[q] = batch.sparse_sectors == nullptr || !takesGatherScan(batch.sparse_sectors + q * SPARSE_COUNTER_STRIDE, batch.sparse_capacity);
   }
   bool any_dense = false;
#pragma unroll
   for (int q = 0; q < Q; ++q) {
      any_dense |= dense[q];
   }
   if (!any_dense) {
      return;
   }

   // this thread's 16-byte chunks of the tile; the filter words stay in registers for all positions
   uint32_t word[CHUNKS];
   ulonglong2 f[Q][CHUNKS];
#pragma unroll
   for (int j = 0; j < CHUNKS; ++j) {
      word[j] = tile * TILE_WORDS + (j * SCAN_THREADS + tid) * 2;
      const bool inside = word[j] < row_words;
      if (!inside) {
         word[j] = 0;  // out-of-row chunks read word 0 (always valid) against zero filters: no branch in the loop
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
         f[q][j] = inside && dense[q] ? *reinterpret_cast<const ulonglong2*>(batch.filters[q] + word[j]) : make_ulonglong2(0, 0);
      }
   }

   // A tile without a selected row has nothing to count: rows laid out by lineage or date (the reference partitions by a
   // key column and orders by date, preprocessor.cpp:159-227) give lineage and date filters long runs of zero words, and such a block leaves before its first load.
   {
      uint64_t any_bit = 0;
#pragma unroll
      for (int j = 0; j < CHUNKS; ++j) {
#pragma unroll
         for (int q = 0; q < Q; ++q) {
            any_bit |= f[q][j].x | f[q][j].y;
         }
      }
      // One-hot rows of a pruning scan: the block's first wave lists the rows of the range that stay — a row is left out where
      // EVERY filter this launch counts allows it (granulePrunable, the escape pass's rule; a filter routed to the gather kernel is
      // counted exactly there and has no say) — while the filter tile is on its way; the barrier below publishes the list.
      // Lane l looks at rows l, l + 64, ...: a row's place in the list is the live rows of the ballots before plus those of
      // the lanes below in its own.  A range that counts the end runs of the gap symbol (batch.row_covered) lists its rows as well,
      // pruning or not: the covered rows are left out for every filter — the escape pass counts them from the end events.
      if constexpr (KIND == KIND_ROWS) {
         const bool by_bounds = rows.heaviest[range] != nullptr;       // (uniform)
         const uint8_t* __restrict__ covered = batch.row_covered[range];  // (uniform)
         if ((by_bounds || covered != nullptr) && n_rows <= ROW_LIST_MAX && tid < 64u) {  // (uniform per wave)
            constexpr uint32_t PER_LANE = ROW_LIST_MAX / 64u;
            uint32_t heaviest[PER_LANE];
            uint32_t without[PER_LANE];
            // the flags first, folded into one register before the bounds are asked for (flags and bounds in flight together
            // would be 48 registers, more than the pipeline of the narrow instantiations needs anywhere else)
            uint32_t left_out = 0;  // bit k: row k * 64 + tid is covered
            if (covered != nullptr) {
#pragma unroll
               for (uint32_t k = 0; k < PER_LANE; ++k) {
                  left_out |= (covered[min(k * 64u + tid, n_rows - 1u)] != 0 ? 1u : 0u) << k;
               }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (uint32_t k = 0; k < PER_LANE; ++k) {  // (unconditional, clamped: all in flight at once)
               const uint32_t row = min(k * 64u + tid, n_rows - 1u);
               heaviest[k] = by_bounds ? rows.heaviest[range][row] : 0xFFFFFFFFu;
               without[k] = by_bounds ? rows.without[range][row] : 0xFFFFFFFFu;
            }
            uint32_t cardinality[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
               cardinality[q] = by_bounds ? rows.counters[q * SPARSE_COUNTER_STRIDE + 2u] : 0u;
            }
            uint32_t n_live = 0;
#pragma unroll
            for (uint32_t k = 0; k < PER_LANE; ++k) {
               const uint32_t row = k * 64u + tid;
               bool skip = by_bounds;
#pragma unroll
               for (int q = 0; q < Q; ++q) {
                  if (dense[q]) {
                     skip = skip && granulePrunable(cardinality[q], without[k], heaviest[k], rows.min_proportion[q]);
                  }
               }
               const bool live = row < n_rows && !skip && ((left_out >> k) & 1u) == 0;
               const uint64_t live_lanes = __ballot(live);
               if (live) {
                  s_live_rows[n_live + static_cast<uint32_t>(__popcll(live_lanes & ((uint64_t{1} << tid) - 1u)))] = row;
               }
               n_live += static_cast<uint32_t>(__popcll(live_lanes));
            }
            if (tid == 0) {
               s_live_rows[ROW_LIST_MAX] = n_live;
            }
         }
      }
      if (__syncthreads_or(any_bit != 0 ? 1 : 0) == 0) {
         return;
      }
   }
   // (the list's entries are the same for every lane: kept in scalar registers, as the escape pass keeps its granules)
   [[maybe_unused]] const auto liveRow = [&](uint32_t k) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_live_rows[k]))); };
   [[maybe_unused]] uint32_t n_live = n_rows;
   bool listed = false;  // (uniform) the block walks the list of live rows, not rows 0 .. n_rows
   if constexpr (KIND == KIND_ROWS) {
      listed = (rows.heaviest[range] != nullptr || batch.row_covered[range] != nullptr) && n_rows <= ROW_LIST_MAX;
      if (listed) {
         // The position groups of the range take even shares of the LIVE pairs, not of all pairs: the rows left out cluster (the
         // flanks of an alignment's ragged ends), all blocks of a launch are resident together, and the launch ends with its
         // slowest group.  A group without a share leaves before its first plane load.
         n_live = liveRow(ROW_LIST_MAX);
         const uint32_t n_groups = (batch.first_unit[range + 1] - batch.first_unit[range]) / n_tiles;
         const uint32_t live_pairs = (n_live + 1u) / 2u;
         pos_begin = static_cast<uint32_t>(static_cast<uint64_t>(position_group) * live_pairs / n_groups);
         pos_end = static_cast<uint32_t>(static_cast<uint64_t>(position_group + 1u) * live_pairs / n_groups);
         if (pos_begin >= pos_end) {
            return;
         }
      }
   }
   const uint32_t last_pos = pos_end - 1;

   // LISTED (a std::bool_constant): the pair of rows of a "position" is taken from the list of live rows
   auto load_position = [&](auto LISTED, uint32_t position, ulonglong2 (&dst)[BITS][CHUNKS]) {
      if constexpr (decltype(LISTED)::value) {
         // the second row of the last pair of an odd list is the first one again (not stored)
         const uint32_t pair[2] = {liveRow(position * 2u), liveRow(min(position * 2u + 1u, n_live - 1u))};
#pragma unroll
         for (int bit = 0; bit < BITS; ++bit) {
            const uint64_t* base = planes + static_cast<size_t>(pair[bit & 1]) * row_words;
#pragma unroll
            for (int j = 0; j < CHUNKS; ++j) {
               dst[bit][j] = loadPlane16<true>(base + word[j]);
            }
         }
      } else {
         const uint64_t* base = planes + static_cast<size_t>(position) * BITS * row_words;
#pragma unroll
         for (int bit = 0; bit < BITS; ++bit) {
            // the second row of the last pair of an odd run is the first one again (in bounds, not stored)
            const size_t row = KIND == KIND_ROWS ? static_cast<size_t>(min(static_cast<uint32_t>(bit), n_rows - 1u - position * 2u)) : static_cast<size_t>(bit);
#pragma unroll
            for (int j = 0; j < CHUNKS; ++j) {
               dst[bit][j] = loadPlane16<true>(base + row * row_words + word[j]);
            }
         }
      }
   };
   auto reduce_position = [&](const ulonglong2 (&src)[BITS][CHUNKS], uint32_t buffer, uint32_t slot, bool store) {
      uint32_t acc[NSYM][Q];
#pragma unroll
      for (int symbol = 0; symbol < NSYM; ++symbol) {
#pragma unroll
         for (int q = 0; q < Q; ++q) {
            acc[symbol][q] = 0;
         }
      }
#pragma unroll
      for (int j = 0; j < CHUNKS; ++j) {
#pragma unroll
         for (int half = 0; half < 2; ++half) {
            uint64_t bits[BITS];
#pragma unroll
            for (int bit = 0; bit < BITS; ++bit) {
               bits[bit] = half == 0 ? src[bit][j].x : src[bit][j].y;
            }
            // Decode tree: the four combinations of the two low code bits, of the next two, and the top bit — a symbol
            // is then two ANDs (22 symbols from 5 planes: ~55 logic ops per word instead of 110).  With one filter the
            // filter is folded into the low pair, so the per-symbol AND with it disappears as well.
            const uint64_t filter0 = half == 0 ? f[0][j].x : f[0][j].y;
            if constexpr (KIND == KIND_ROWS) {
#pragma unroll
               for (int row = 0; row < NSYM; ++row) {
#pragma unroll
                  for (int q = 0; q < Q; ++q) {
                     acc[row][q] += static_cast<uint32_t>(__popcll(bits[row] & (half == 0 ? f[q][j].x : f[q][j].y)));
                  }
               }
               continue;
            }
            uint64_t low[4];
            low[0] = ~bits[1] & ~bits[0];
            low[1] = ~bits[1] & bits[0];
            low[2] = bits[1] & ~bits[0];
            low[3] = bits[1] & bits[0];
            if constexpr (Q == 1) {
#pragma unroll
               for (int k = 0; k < 4; ++k) {
                  low[k] &= filter0;
               }
            }
            uint64_t high[BITS <= 3 ? 2 : 8];
            static_assert(NSYM < (1 << BITS), "every counted code needs a bit pattern of its own, 0 is 'none'");
            if constexpr (BITS == 2) {
               high[0] = ~0ull;  // the codes ARE the low pair
               high[1] = 0;
            } else if constexpr (BITS == 3) {
               high[0] = ~bits[2];
               high[1] = bits[2];
            } else {
               static_assert(BITS == 5, "decode tree written for 2, 3 or 5 code bits");
#pragma unroll
               for (int k = 0; k < 8; ++k) {
                  high[k] = ((k & 1) != 0 ? bits[2] : ~bits[2]) & ((k & 2) != 0 ? bits[3] : ~bits[3]) & ((k & 4) != 0 ? bits[4] : ~bits[4]);
               }
            }
#pragma unroll
            for (int symbol = 0; symbol < NSYM; ++symbol) {
               const uint32_t code = static_cast<uint32_t>(symbol) + 1u;
               const uint64_t match = BITS == 2 ? low[code & 3u] : (low[code & 3u] & high[code >> 2]);
#pragma unroll
               for (int q = 0; q < Q; ++q) {
                  const uint64_t filter_word = half == 0 ? f[q][j].x : f[q][j].y;
                  acc[symbol][q] += static_cast<uint32_t>(__popcll(Q == 1 ? match : (match & filter_word)));
               }
            }
         }
      }
      // wave reduction, two symbols per register: a lane counted at most WPT * 64 <= 512 rows per symbol, so a wave total
      // fits 16 bits (<= 32 768) and the 6 DPP steps serve two symbols at once
      static_assert(WPT * 64 * 64 < 65536, "packed wave totals need 16 bits per symbol");
#pragma unroll
      for (int symbol = 0; symbol < NSYM; symbol += 2) {
#pragma unroll
         for (int q = 0; q < Q; ++q) {
            const bool pair = symbol + 1 < NSYM;
            const uint32_t packed = pair ? (acc[symbol][q] | (acc[symbol + 1 < NSYM ? symbol + 1 : symbol][q] << 16)) : acc[symbol][q];
            const uint32_t total = waveSumToLane63(packed);
            if (writer && store) {
               s_partial[buffer][wave][slot][q * NSYM + symbol] = pair ? (total & 0xFFFFu) : total;
               if (pair) {
                  s_partial[buffer][wave][slot][q * NSYM + symbol + 1] = total >> 16;
               }
            }
         }
      }
   };
   auto flush = [&](auto LISTED, uint32_t batch_first_position, uint32_t n_batch, uint32_t buffer) {
      __syncthreads();
      for (uint32_t item = tid; item < n_batch * (NSYM * Q); item += SCAN_THREADS) {
         const uint32_t position = item / (NSYM * Q);
         const uint32_t rest = item % (NSYM * Q);
         uint32_t total = 0;
#pragma unroll
         for (int w = 0; w < SCAN_WAVES; ++w) {
            total += s_partial[buffer][w][position][rest];
         }
         if (total != 0) {
            if constexpr (KIND == KIND_ROWS) {  // row -> its (position, symbol) counter
               uint32_t row = (batch_first_position + position) * 2u + rest % NSYM;
               if constexpr (decltype(LISTED)::value) {
                  row = row < n_live ? s_live_rows[row] : n_rows;
               }
               if (row < n_rows) {
                  const uint32_t target = reinterpret_cast<const uint32_t*>(batch.code_map[range])[row] - batch.target_base[range];
                  atomicAdd(&batch.counts[range][rest / NSYM][target], total);
               }
            } else if constexpr (KIND == KIND_MAPPED) {  // code -> the symbol it stands for at this position
               const uint32_t symbol = batch.code_map[range][static_cast<size_t>(batch_first_position + position) * CODE_MAP_STRIDE + 1 + rest % NSYM];
               if (symbol < batch.out_symbols) {  // an unused code (0xFF) has no rows: never taken, never out of bounds
                  atomicAdd(&batch.counts[range][rest / NSYM][static_cast<size_t>(batch_first_position + position) * batch.out_symbols + symbol], total);
               }
            } else {
               atomicAdd(&batch.counts[range][rest / NSYM][static_cast<size_t>(batch_first_position + position) * NSYM + rest % NSYM], total);
            }
         }
      }
   };

   auto scan_positions = [&](auto LISTED) {
      ulonglong2 buf_a[BITS][CHUNKS];
      ulonglong2 buf_b[BITS][CHUNKS];
      load_position(LISTED, pos_begin, buf_a);
      uint32_t buffer = 0;
      uint32_t batch_first_position = pos_begin;
      for (uint32_t position = pos_begin; position < pos_end; position += 2) {
         load_position(LISTED, min(position + 1, last_pos), buf_b);
         reduce_position(buf_a, buffer, position - batch_first_position, true);
         load_position(LISTED, min(position + 2, last_pos), buf_a);
         reduce_position(buf_b, buffer, position + 1 - batch_first_position, position + 1 < pos_end);
         const uint32_t done = min(position + 2, pos_end) - batch_first_position;
         if (done >= static_cast<uint32_t>(POS_BATCH) || position + 2 >= pos_end) {  // POS_BATCH is even
            flush(LISTED, batch_first_position, done, buffer);
            batch_first_position += done;
            buffer ^= 1u;
         }
      }
   };
   if constexpr (KIND == KIND_ROWS) {
      if (listed) {
         scan_positions(std::true_type{});
         return;
      }
   }
   scan_positions(std::false_type{});
}

// ------------------------------------------------------------------------------------------------
// K1b: one wave per position, for short rows (small N) where a 256-thread column tile would be mostly empty.
// ------------------------------------------------------------------------------------------------
template <int BITS, int NSYM>
__global__ __launch_bounds__(256) void k_scan_sliced_rowwave(
   const uint64_t* __restrict__ planes, const uint64_t* __restrict__ filter, uint32_t* __restrict__ counts, uint32_t row_words,
   uint32_t n_positions
) {
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
   const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
   for (uint32_t position = wave; position < n_positions; position += n_waves) {
      const uint64_t* base = planes + static_cast<size_t>(position) * BITS * row_words;
      uint32_t acc[NSYM];
#pragma unroll
      for (int symbol = 0; symbol < NSYM; ++symbol) {
         acc[symbol] = 0;
      }
      for (uint32_t w = lane; w < row_words; w += 64) {
         const uint64_t filter_word = filter[w];
         uint64_t bits[BITS];
#pragma unroll
         for (int bit = 0; bit < BITS; ++bit) {
            bits[bit] = base[static_cast<size_t>(bit) * row_words + w];
         }
#pragma unroll
         for (int symbol = 0; symbol < NSYM; ++symbol) {
            const uint32_t code = static_cast<uint32_t>(symbol) + 1u;
            uint64_t match = filter_word;
#pragma unroll
            for (int bit = 0; bit < BITS; ++bit) {
               match &= ((code >> bit) & 1u) != 0 ? bits[bit] : ~bits[bit];
            }
            acc[symbol] += static_cast<uint32_t>(__popcll(match));
         }
      }
#pragma unroll
      for (int symbol = 0; symbol < NSYM; ++symbol) {
         const uint32_t total = waveSumToLane63(acc[symbol]);
         if (lane == 63u && total != 0) {
            atomicAdd(&counts[static_cast<size_t>(position) * NSYM + symbol], total);
         }
      }
   }
}

// ------------------------------------------------------------------------------------------------
// K1s: Mutations scan under a SPARSE filter.  The dense scan costs the same whatever the filter selects; the reference's
// roaring and_cardinality gets cheaper with the filter (mutations.cpp:139-164 over a small filter bitmap), so a query
// for a few hundred rows must not pay for 112 GB.  k_compact_filter lists the 64-byte SECTORS (8 consecutive words —
// the unit HBM delivers) of the filter that hold a set bit, at most `capacity` of them (the total is counted
// regardless); when they fit, k_scan_gather reads only those sectors of every plane and k_scan_sliced skips the
// filter.  The decision is taken on the device from the counters (takesGatherScan): no host round trip.  Measured at 10 M
// sequences (profiles/r01_sparse_filters.md, r02_one_hot_rows.md): ~0.9 µs per listed sector of the genome against 6 ms for
// the dense scan, hence the default capacity of row_words / 16 sectors.
// ------------------------------------------------------------------------------------------------

/// Also the scan's "prepare" step (one launch in front of everything else): the blocks zero `n_zero_words` words of scratch
/// (the private count tables of a scan with derived symbols) between them, add the filter's cardinality to counter [2], and
/// block (0, 0) zeroes the counter set the NEXT scan on this scratch block will use (the sets alternate: no fill launches).
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_filter(
   const ScanBatchArgs batch, uint32_t row_words, uint32_t capacity, uint32_t* __restrict__ sparse_sectors, uint32_t* __restrict__ sector_index,
   uint32_t* __restrict__ zero_words, uint32_t n_zero_words, uint32_t* __restrict__ counters_to_reset
) {
   __shared__ uint32_t s_wave_first[COMPACT_THREADS / 64];
   __shared__ uint32_t s_wave_rows[COMPACT_THREADS / 64];
   __shared__ uint32_t s_block_first;
   const uint32_t q = blockIdx.y;
   const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;  // row_words is a multiple of 32: sectors never straddle the row end
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t wave = threadIdx.x >> 6;
   const uint64_t value = w < row_words ? batch.filters[q][w] : 0;
   {  // this block's share of the scratch to zero (16-byte stores; n_zero_words is a multiple of 4)
      const uint32_t n_chunks = n_zero_words / 4u;
      const uint32_t n_threads = gridDim.x * gridDim.y * COMPACT_THREADS;
      for (uint32_t chunk = (blockIdx.y * gridDim.x + blockIdx.x) * COMPACT_THREADS + threadIdx.x; chunk < n_chunks; chunk += n_threads) {
         reinterpret_cast<uint4*>(zero_words)[chunk] = make_uint4(0, 0, 0, 0);
      }
      if (blockIdx.x == 0 && blockIdx.y == 0 && counters_to_reset != nullptr && threadIdx.x < SILO_GPU_MAX_SCAN_BATCH * SPARSE_COUNTER_STRIDE) {
         counters_to_reset[threadIdx.x] = 0;
      }
   }
   const uint64_t ballot = __ballot(value != 0);
   // one bit per sector of this wave (at the sector's first lane): does any of its 8 words have a set bit?
   uint64_t leaders = 0;
#pragma unroll
   for (uint32_t sector = 0; sector < 64 / SECTOR_WORDS; ++sector) {
      if (((ballot >> (sector * SECTOR_WORDS)) & 0xFFull) != 0) {
         leaders |= 1ull << (sector * SECTOR_WORDS);
      }
   }
   const uint32_t wave_rows = waveSumToLane63(static_cast<uint32_t>(__popcll(value)));
   if (lane == 0) {
      s_wave_first[wave] = static_cast<uint32_t>(__popcll(leaders));
   }
   if (lane == 63u) {
      s_wave_rows[wave] = wave_rows;
   }
   __syncthreads();
   if (threadIdx.x == 0) {  // exclusive prefix over the waves, ONE atomic per block
      uint32_t total = 0;
      uint32_t rows = 0;
      for (uint32_t k = 0; k < COMPACT_THREADS / 64; ++k) {
         const uint32_t count = s_wave_first[k];
         s_wave_first[k] = total;
         total += count;
         rows += s_wave_rows[k];
      }
      s_block_first = total != 0 ? atomicAdd(sparse_sectors + q * SPARSE_COUNTER_STRIDE, total) : 0;
      if (total != 0) {
         atomicAdd(sparse_sectors + q * SPARSE_COUNTER_STRIDE + 1, 1u);  // stretches of COMPACT_THREADS words with a set bit
         atomicAdd(sparse_sectors + q * SPARSE_COUNTER_STRIDE + 2, rows);  // the filter's cardinality
      }
   }
   __syncthreads();
   if (((leaders >> lane) & 1ull) != 0) {
      const uint32_t slot = s_block_first + s_wave_first[wave] + static_cast<uint32_t>(__popcll(leaders & ((1ull << lane) - 1ull)));
      if (slot < capacity) {
         sector_index[static_cast<size_t>(q) * capacity + slot] = w / SECTOR_WORDS;
      }
   }
}

// One WAVE per group of POSG consecutive positions (no LDS, no block-level reduction: a sparse filter may have fewer
// non-zero words than a block has lanes); lanes stride over the words of the listed sectors, POSG * BITS gathers in flight each.
template <int BITS, int NSYM, int POSG, int KIND>
__global__ __launch_bounds__(256, (BITS <= 3 ? (NSYM <= 5 ? 5 : 4) : 4)) void k_scan_gather(
   const ScanBatchArgs batch, const uint32_t* __restrict__ sector_index, uint32_t capacity, uint32_t row_words
) {
   const uint32_t q = blockIdx.y;
   const uint32_t n_sectors = batch.sparse_sectors[q * SPARSE_COUNTER_STRIDE];
   if (n_sectors == 0 || !takesGatherScan(batch.sparse_sectors + q * SPARSE_COUNTER_STRIDE, batch.sparse_capacity)) {
      return;  // empty filter, or a dense one (k_scan_sliced has it); `capacity` is the stride of the lists
   }
   const uint32_t n_words = n_sectors * SECTOR_WORDS;
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t unit = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // this wave
   if (unit >= batch.first_unit[batch.n_ranges]) {
      return;
   }
   uint32_t range = 0;
   while (range + 1 < batch.n_ranges && unit >= batch.first_unit[range + 1]) {
      ++range;
   }
   const uint64_t* __restrict__ planes = batch.planes[range];
   static_assert(KIND != KIND_ROWS || (BITS == 1 && NSYM == 1), "one-hot rows are gathered one by one");
   const uint32_t n_positions = batch.n_positions[range];  // KIND_ROWS: plane rows
   const uint32_t pos_begin = (unit - batch.first_unit[range]) * POSG;
   const uint32_t last_pos = n_positions - 1;
   const uint32_t* index = sector_index + static_cast<size_t>(q) * capacity;
   const uint64_t* filter = batch.filters[q];
   const size_t position_stride = static_cast<size_t>(BITS) * row_words;
   // one-hot rows of a range that counts the end runs of the gap symbol: the covered rows are left out here as k_scan_sliced
   // leaves them out (the same flags; uniform per wave)
   [[maybe_unused]] uint32_t left_out = 0;  // bit g: row pos_begin + g is covered
   if constexpr (KIND == KIND_ROWS) {
      if (batch.row_covered[range] != nullptr) {
#pragma unroll
         for (int g = 0; g < POSG; ++g) {
            left_out |= (batch.row_covered[range][min(pos_begin + g, last_pos)] != 0 ? 1u : 0u) << g;
         }
         left_out = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(left_out)));
         if (left_out == (1u << POSG) - 1u) {
            return;
         }
      }
   }

   uint32_t acc[POSG][NSYM];
#pragma unroll
   for (int g = 0; g < POSG; ++g) {
#pragma unroll
      for (int symbol = 0; symbol < NSYM; ++symbol) {
         acc[g][symbol] = 0;
      }
   }
   for (uint32_t i = lane; i < n_words; i += 64) {
      const uint32_t w = index[i / SECTOR_WORDS] * SECTOR_WORDS + i % SECTOR_WORDS;  // 8 lanes share a 64-byte sector
      const uint64_t filter_word = filter[w];
      uint64_t bits[POSG][BITS];
#pragma unroll
      for (int g = 0; g < POSG; ++g) {
         // positions past the end are clamped (an in-bounds re-read) and not stored below
         const uint64_t* base = planes + static_cast<size_t>(min(pos_begin + g, last_pos)) * position_stride + w;
#pragma unroll
         for (int bit = 0; bit < BITS; ++bit) {
            bits[g][bit] = KIND == KIND_ROWS && ((left_out >> g) & 1u) != 0 ? 0ull : base[static_cast<size_t>(bit) * row_words];
         }
      }
#pragma unroll
      for (int g = 0; g < POSG; ++g) {
         if constexpr (KIND == KIND_ROWS) {
            acc[g][0] += static_cast<uint32_t>(__popcll(bits[g][0] & filter_word));
            continue;
         }
         constexpr int B1 = BITS > 1 ? 1 : 0;  // (one plane: never decoded)
         uint64_t low[4];
         low[0] = ~bits[g][B1] & ~bits[g][0] & filter_word;
         low[1] = ~bits[g][B1] & bits[g][0] & filter_word;
         low[2] = bits[g][B1] & ~bits[g][0] & filter_word;
         low[3] = bits[g][B1] & bits[g][0] & filter_word;
         uint64_t high[BITS <= 3 ? 2 : 8];
         if constexpr (BITS <= 2) {
            high[0] = ~0ull;  // the codes are the low pair
            high[1] = 0;
         } else if constexpr (BITS == 3) {
            high[0] = ~bits[g][2];
            high[1] = bits[g][2];
         } else if constexpr (BITS == 5) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
               high[k] = ((k & 1) != 0 ? bits[g][2] : ~bits[g][2]) & ((k & 2) != 0 ? bits[g][3] : ~bits[g][3]) &
                         ((k & 4) != 0 ? bits[g][4] : ~bits[g][4]);
            }
         }
#pragma unroll
         for (int symbol = 0; symbol < NSYM; ++symbol) {
            const uint32_t code = static_cast<uint32_t>(symbol) + 1u;
            acc[g][symbol] += static_cast<uint32_t>(__popcll(BITS <= 2 ? low[code & 3u] : (low[code & 3u] & high[code >> 2])));
         }
      }
   }
#pragma unroll
   for (int g = 0; g < POSG; ++g) {
#pragma unroll
      for (int symbol = 0; symbol < NSYM; ++symbol) {
         const uint32_t total = waveSumToLane63(acc[g][symbol]);
         if (lane == 63u && total != 0 && pos_begin + g < n_positions) {
            if constexpr (KIND == KIND_ROWS) {  // row -> its (position, symbol) counter
               const uint32_t target = reinterpret_cast<const uint32_t*>(batch.code_map[range])[pos_begin + g] - batch.target_base[range];
               atomicAdd(&batch.counts[range][q][target], total);
            } else if constexpr (KIND == KIND_MAPPED) {  // code -> the symbol it stands for at this position
               const uint32_t mapped = batch.code_map[range][static_cast<size_t>(pos_begin + g) * CODE_MAP_STRIDE + 1 + symbol];
               if (mapped < batch.out_symbols) {
                  atomicAdd(&batch.counts[range][q][static_cast<size_t>(pos_begin + g) * batch.out_symbols + mapped], total);
               }
            } else {
               atomicAdd(&batch.counts[range][q][static_cast<size_t>(pos_begin + g) * NSYM + symbol], total);
            }
         }
      }
   }
}

/// Launches k_scan_sliced for the `q_count` filters and the pieces already entered in `batch` (planes, n_positions, counts).
/// `rows`: what a launch over one-hot rows may leave rows out by (all null otherwise).  Such a launch is named "..., pruning" in the
/// timing log, as the key pass is; its plane_rows and bytes stay those of ALL its rows, whatever it skips.
template <int BITS, int NSYM, int KIND>
int launchSlicedScan(ScanBatchArgs& batch, const RowPruneArgs& rows, uint32_t row_words, uint32_t q_count, hipStream_t hip_stream) {
   // words per thread: 8 for one filter over a layout of at most 5 counted symbols (2 or 3 planes x 4 chunks per position and
   // buffer), 4 otherwise (7 or 22 symbols; batches: Q filter tiles in registers).  SILO_GPU_TUNE_SCAN_VARIANT 10 / 12 force 4 / 8.
   const int variant = g_tune_scan_variant.load();
   constexpr bool CAN_BE_WIDE = BITS <= 3;
   bool wide = CAN_BE_WIDE && q_count == 1 && row_words >= SCAN_THREADS * 8;
   if (variant == 10) {
      wide = false;
   } else if (variant == 12 && CAN_BE_WIDE && q_count == 1) {
      wide = true;
   }
   const uint32_t tile_words = SCAN_THREADS * (wide ? 8 : 4);
   int positions_per_block = g_tune_rows_per_block.load();
   const uint32_t n_tiles = (row_words + tile_words - 1) / tile_words;
   // what the pipeline steps through: positions of BITS planes, or pairs of one-hot rows
   const auto units = [&](uint32_t r) { return KIND == KIND_ROWS ? (batch.n_positions[r] + 1u) / 2u : batch.n_positions[r]; };
   uint64_t total_positions = 0;
   for (uint32_t r = 0; r < batch.n_ranges; ++r) {
      total_positions += units(r);
   }
   if (positions_per_block <= 0) {
      // 2 or 3 planes per position: 128 positions per block while that still leaves >= 4096 blocks, else 64; the 5 identity
      // planes of amino acids: 12 (60 plane rows) — profiles/r01_scan_variants.md
      // (a block re-reads its filter tile — one plane row's worth — whatever it scans, so fewer positions per block cost
      // 1 / (positions x planes) more bytes; too few blocks leave the chip idle at the launch's tail)
      positions_per_block = 12;
      if constexpr (BITS <= 3) {
         positions_per_block = 128;
         while (positions_per_block > 32 && static_cast<uint64_t>(n_tiles) * ((total_positions + positions_per_block - 1) / positions_per_block) < 12288) {
            positions_per_block /= 2;
         }
      }
   }
   positions_per_block += positions_per_block & 1;  // the pipeline works on pairs of positions
   batch.first_unit[0] = 0;
   for (uint32_t r = 0; r < batch.n_ranges; ++r) {
      batch.first_unit[r + 1] = batch.first_unit[r] + n_tiles * ((units(r) + positions_per_block - 1) / positions_per_block);
   }
   const dim3 grid(batch.first_unit[batch.n_ranges]);
   ScanLaunchTiming* timing = nullptr;
   if (g_tune_scan_timing.load() == 1) {
      uint64_t plane_rows = 0;
      for (uint32_t r = 0; r < batch.n_ranges; ++r) {
         plane_rows += KIND == KIND_ROWS ? batch.n_positions[r] : static_cast<uint64_t>(batch.n_positions[r]) * BITS;
      }
      bool bounds = false, ends = false;
      for (uint32_t r = 0; r < batch.n_ranges; ++r) {
         bounds = bounds || (KIND == KIND_ROWS && rows.heaviest[r] != nullptr);
         ends = ends || (KIND == KIND_ROWS && batch.row_covered[r] != nullptr);
      }
      char name[64];
      std::snprintf(name, sizeof(name), "k_scan_sliced<%d, %d, %d, %u, %d>%s%s", BITS, NSYM, wide ? 8 : 4, wide ? 1u : std::min(q_count, 8u), KIND, bounds ? ", pruning" : "",
                    ends ? ", ends" : "");
      timing = startLaunchTiming(name, plane_rows, (plane_rows + q_count) * row_words * sizeof(uint64_t), q_count, grid.x, hip_stream);
   }
#define SILO_LAUNCH_SLICED(WPT, Q) \
   k_scan_sliced<BITS, NSYM, WPT, Q, KIND><<<grid, SCAN_THREADS, 0, hip_stream>>>(batch, rows, row_words, positions_per_block, n_tiles)
   if (wide) {
      if constexpr (CAN_BE_WIDE) {
         SILO_LAUNCH_SLICED(8, 1);
      }
   } else {
      switch (q_count) {
         case 1: SILO_LAUNCH_SLICED(4, 1); break;
         case 2: SILO_LAUNCH_SLICED(4, 2); break;
         case 3: SILO_LAUNCH_SLICED(4, 3); break;
         case 4: SILO_LAUNCH_SLICED(4, 4); break;
         default:
            if constexpr (NSYM <= 5) {  // 5..8 filters: layouts of at most 5 counted symbols (the others go in groups of 4)
               switch (q_count) {
                  case 5: SILO_LAUNCH_SLICED(4, 5); break;
                  case 6: SILO_LAUNCH_SLICED(4, 6); break;
                  case 7: SILO_LAUNCH_SLICED(4, 7); break;
                  default: SILO_LAUNCH_SLICED(4, 8); break;
               }
            } else {
               return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "launchSlicedScan: more than 4 filters in one pass over a 7- or 22-symbol layout");
            }
      }
   }
#undef SILO_LAUNCH_SLICED
   HIP_TRY(hipGetLastError());
   finishLaunchTiming(timing, hip_stream);
   return SILO_GPU_OK;
}

/// Launches k_scan_gather (one wave per POSG positions) for the pieces in `batch`; grid.y = filter.
template <int BITS, int NSYM, int POSG, int KIND>
int launchGatherScan(ScanBatchArgs& batch, const uint32_t* sector_index, uint32_t stride, uint32_t row_words, uint32_t q_count, hipStream_t hip_stream) {
   batch.first_unit[0] = 0;
   for (uint32_t r = 0; r < batch.n_ranges; ++r) {
      batch.first_unit[r + 1] = batch.first_unit[r] + (batch.n_positions[r] + POSG - 1) / POSG;
   }
   const uint32_t waves = batch.first_unit[batch.n_ranges];
   k_scan_gather<BITS, NSYM, POSG, KIND><<<dim3((waves + 3) / 4, q_count), 256, 0, hip_stream>>>(batch, sector_index, stride, row_words);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

/// The launch descriptor of filters [first_filter, first_filter + n_filters) over pieces[first_piece, ...), SCAN_MAX_RANGES at the most.
/// sparse_sectors: the routing counters of the scan's first filter, or nullptr.
ScanBatchArgs pieceBatch(
   const std::vector<ScanPiece>& pieces, size_t first_piece, const SeqStoreDev& any_store, const uint64_t* const* filters, uint32_t first_filter,
   uint32_t n_filters, const uint32_t* sparse_sectors, uint32_t sparse_capacity
) {
   ScanBatchArgs batch{};
   batch.sparse_sectors = sparse_sectors != nullptr ? sparse_sectors + first_filter * SPARSE_COUNTER_STRIDE : nullptr;
   batch.sparse_capacity = sparse_capacity;
   batch.out_symbols = any_store.n_scan;
   copyFilters(batch.filters, filters + first_filter, n_filters);
   batch.n_ranges = static_cast<uint32_t>(std::min<size_t>(SCAN_MAX_RANGES, pieces.size() - first_piece));
   for (uint32_t r = 0; r < batch.n_ranges; ++r) {
      const ScanPiece& piece = pieces[first_piece + r];
      batch.planes[r] = piece.planes;
      batch.code_map[r] = piece.code_map;
      batch.target_base[r] = piece.target_base;
      batch.row_covered[r] = piece.row_covered;
      batch.n_positions[r] = piece.n_positions;
      std::copy_n(piece.counts + first_filter, n_filters, batch.counts[r]);
   }
   return batch;
}

}  // namespace

namespace silo_gpu_detail {

/// Short rows (fewer words than one column tile): one wave per position over the identity planes (such stores keep them), one
/// filter and one range at a time.
int scanShortRows(const std::vector<ScanRange>& ranges, bool nucleotide, const uint64_t* const* filters, uint32_t q_count, hipStream_t hip_stream) {
   for (const ScanRange& range : ranges) {
      const SeqStoreDev& dev = range.seqstore->dev;
      const uint32_t n_positions = range.pos_end - range.pos_begin;
      const uint32_t waves = std::min<uint32_t>(n_positions, 256u * 32u);
      const uint32_t blocks = (waves + 3) / 4;
      const uint64_t* planes = dev.planes + static_cast<size_t>(range.pos_begin) * dev.n_bits * dev.row_words;
      for (uint32_t q = 0; q < q_count; ++q) {
         if (nucleotide) {
            k_scan_sliced_rowwave<3, 5><<<blocks, 256, 0, hip_stream>>>(planes, filters[q], range.counts[q], dev.row_words, n_positions);
         } else {
            k_scan_sliced_rowwave<5, 22><<<blocks, 256, 0, hip_stream>>>(planes, filters[q], range.counts[q], dev.row_words, n_positions);
         }
      }
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

/// The prepare step (k_compact_filter): the sectors of every filter that hold a set bit, its cardinality, `table_words` words of
/// `tables` zeroed, the other counter set re-armed.
hipError_t prepareScan(
   const uint64_t* const* filters, uint32_t q_count, uint32_t row_words, uint32_t capacity, uint32_t* counters, uint32_t* sector_index, uint32_t* tables,
   uint32_t table_words, uint32_t* counters_to_reset, hipStream_t hip_stream
) {
   ScanBatchArgs compact{};
   copyFilters(compact.filters, filters, q_count);
   k_compact_filter<<<dim3((row_words + COMPACT_THREADS - 1) / COMPACT_THREADS, q_count), COMPACT_THREADS, 0, hip_stream>>>(
      compact, row_words, capacity, counters, sector_index, tables, table_words, counters_to_reset
   );
   return hipGetLastError();
}

/// The dense kernels for `q_count` filters over the pieces of every layout: at most SCAN_MAX_RANGES pieces and 8 (layouts
/// of 3 or 5 counted symbols) or 4 (7 or 22) filters per launch.  sparse_sectors carries the routing counters (or nullptr).
/// With pruning->rows the launches over one-hot rows may leave out the rows that no Mutations row of the filters' proportions can
/// come from, where the store has the bounds for it — where and as scanEscapes leaves out granules of keys.
int scanPiecesDense(
   const std::vector<ScanPiece> (&pieces)[N_SCAN_LAYOUTS], const SeqStoreDev& any_store, const uint64_t* const* filters, uint32_t q_count,
   const uint32_t* sparse_sectors, uint32_t sparse_capacity, hipStream_t hip_stream, const ScanPruning* pruning
) {
   // (running the plane scans of a query's smaller layouts on side streams beside the largest one was tried: no gain, the
   // launches are bandwidth-bound together — profiles/r02_amino_acid.md)
   for (int layout = 0; layout < N_SCAN_LAYOUTS; ++layout) {
      const std::vector<ScanPiece>& list = pieces[layout];
      const uint32_t filters_per_pass = layout == SCAN_2_PLANES || layout == SCAN_FULL_NUCLEOTIDE || layout == SCAN_ONE_HOT_ROWS ? SILO_GPU_MAX_SCAN_BATCH : 4;
      for (size_t first_piece = 0; first_piece < list.size(); first_piece += SCAN_MAX_RANGES) {
         for (uint32_t first = 0; first < q_count; first += filters_per_pass) {
            const uint32_t n = std::min<uint32_t>(filters_per_pass, q_count - first);
            ScanBatchArgs batch = pieceBatch(list, first_piece, any_store, filters, first, n, sparse_sectors, sparse_capacity);
            RowPruneArgs rows{};
            if (pruning != nullptr && pruning->rows && layout == SCAN_ONE_HOT_ROWS) {
               rows.counters = pruning->counters + first * SPARSE_COUNTER_STRIDE;
               std::copy_n(pruning->min_proportion + first, n, rows.min_proportion);
               for (uint32_t r = 0; r < batch.n_ranges; ++r) {
                  rows.heaviest[r] = list[first_piece + r].row_heaviest;
                  rows.without[r] = list[first_piece + r].row_without;
               }
            }
            int rc = SILO_GPU_OK;
            switch (layout) {
               case SCAN_2_PLANES: rc = launchSlicedScan<2, 3, KIND_MAPPED>(batch, rows, any_store.row_words, n, hip_stream); break;
               case SCAN_3_PLANES_MAPPED: rc = launchSlicedScan<3, 7, KIND_MAPPED>(batch, rows, any_store.row_words, n, hip_stream); break;
               case SCAN_FULL_NUCLEOTIDE: rc = launchSlicedScan<3, 5, KIND_IDENTITY>(batch, rows, any_store.row_words, n, hip_stream); break;
               case SCAN_ONE_HOT_ROWS: rc = launchSlicedScan<2, 2, KIND_ROWS>(batch, rows, any_store.row_words, n, hip_stream); break;
               default: rc = launchSlicedScan<5, 22, KIND_IDENTITY>(batch, rows, any_store.row_words, n, hip_stream); break;
            }
            if (rc != SILO_GPU_OK) {
               return rc;
            }
         }
      }
   }
   return SILO_GPU_OK;
}

/// The gather over the sectors of the sparse filters (`sector_index`: `stride` of them per filter), over the same pieces of the
/// same planes as scanPiecesDense.
int scanPiecesGather(
   const std::vector<ScanPiece> (&pieces)[N_SCAN_LAYOUTS], const SeqStoreDev& any_store, const uint64_t* const* filters, uint32_t q_count,
   const uint32_t* sparse_sectors, uint32_t sparse_capacity, const uint32_t* sector_index, uint32_t stride, hipStream_t hip_stream
) {
   for (int layout = 0; layout < N_SCAN_LAYOUTS; ++layout) {
      const std::vector<ScanPiece>& list = pieces[layout];
      for (size_t first_piece = 0; first_piece < list.size(); first_piece += SCAN_MAX_RANGES) {
         ScanBatchArgs batch = pieceBatch(list, first_piece, any_store, filters, 0, q_count, sparse_sectors, sparse_capacity);
         int rc = SILO_GPU_OK;
         switch (layout) {
            case SCAN_2_PLANES: rc = launchGatherScan<2, 3, 4, KIND_MAPPED>(batch, sector_index, stride, any_store.row_words, q_count, hip_stream); break;
            case SCAN_3_PLANES_MAPPED: rc = launchGatherScan<3, 7, 4, KIND_MAPPED>(batch, sector_index, stride, any_store.row_words, q_count, hip_stream); break;
            case SCAN_FULL_NUCLEOTIDE: rc = launchGatherScan<3, 5, 4, KIND_IDENTITY>(batch, sector_index, stride, any_store.row_words, q_count, hip_stream); break;
            case SCAN_ONE_HOT_ROWS: rc = launchGatherScan<1, 1, 8, KIND_ROWS>(batch, sector_index, stride, any_store.row_words, q_count, hip_stream); break;
            default: rc = launchGatherScan<5, 22, 2, KIND_IDENTITY>(batch, sector_index, stride, any_store.row_words, q_count, hip_stream); break;
         }
         if (rc != SILO_GPU_OK) {
            return rc;
         }
      }
   }
   return SILO_GPU_OK;
}

}  // namespace silo_gpu_detail
