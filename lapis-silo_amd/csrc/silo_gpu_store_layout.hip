// silo_gpu_store_layout.hip — finalize: the layout of every position (layout_choice.h) and the adaptive planes with their escape
// keys, re-encoded from the build-time planes or taken over from the encoding pass of a two-pass build.  DESIGN.md section 3.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_internal.h"

using namespace silo_gpu_detail;

// ------------------------------------------------------------------------------------------------
// The adaptive planes.  At almost every position of a real alignment ONE symbol has nearly every row, and where not, three
// symbols cover all but a handful (the reference symbol, the gap or a lineage's substitution, one more), so a finalized store
// does not keep the ceil(log2(|valid| + 1)) code planes of the build (3 nucleotide, 5 amino-acid) everywhere: finalize() picks,
// per POSITION, the cheapest of
//    one-hot rows: 1, 2 or 3 rows, row j = the rows of the position's j-th most frequent valid symbol,
//    2 planes: codes 1..3 = the three most frequent valid symbols of the position,
//    3 planes: codes 1..7 = the seven most frequent (amino acids only: for nucleotides that is the full set),
//    the full identity planes,
// where the rows whose valid symbol the position does not store become explicit keys ("escapes": position << 37 | scan
// symbol << 32 | sequence, sorted; a second copy slice-major for the scan's escape pass).  Cost model (chooseLayouts in
// layout_choice.h, on the host from the unfiltered totals), in bytes the Mutations scan has to move: rows x row bytes +
// KEY_COST_BYTES per escape, the 22-symbol decode of the full amino-acid planes weighted by what it costs in VALU time, and a
// charge per change of layout between neighbouring positions: a scan launch takes runs of ONE layout (one-hot positions of
// any number of rows are one layout: a run of rows), and a run of a few positions costs its blocks the filter tile and the
// pipeline ramp all over again.  The build-time planes are freed afterwards: at 10 M sequences the nucleotide store shrinks
// from 112 GB to 38 GB of plane rows (+ 37 GB for the missing-symbol plane) and every consumer — the scan, the
// sparse-filter gather, filter leaves, FastaAligned — reads the adaptive planes.
// ------------------------------------------------------------------------------------------------
using silo_gpu_layout::KEY_COST_BYTES;

namespace {

/// Re-encodes the build-time planes of every position into its adaptive layout; rows without a code go, with an atomic
/// cursor per (position, symbol), into that counter's exactly sized slice of the key list (sorted afterwards).
template <int BITS>
__global__ __launch_bounds__(256) void k_encode_adaptive(
   const uint64_t* __restrict__ scan, uint32_t row_words, uint32_t n_scan, const uint8_t* __restrict__ code_map, const uint32_t* __restrict__ row_of,
   const uint32_t* __restrict__ escape_first, uint32_t* __restrict__ escape_cursor, uint64_t* __restrict__ planes, uint64_t* __restrict__ escapes
) {
   const uint32_t p = blockIdx.y;
   const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
   if (w >= row_words) {
      return;
   }
   uint64_t bits[BITS];
   uint64_t valid = 0;
#pragma unroll
   for (int bit = 0; bit < BITS; ++bit) {
      bits[bit] = scan[(static_cast<size_t>(p) * BITS + bit) * row_words + w];
      valid |= bits[bit];
   }
   const uint8_t* map = code_map + static_cast<size_t>(p) * CODE_MAP_STRIDE;
   uint64_t* out = planes + static_cast<size_t>(row_of[p]) * row_words + w;
   if ((map[0] & LAYOUT_IDENTITY) != 0) {
#pragma unroll
      for (int bit = 0; bit < BITS; ++bit) {
         out[static_cast<size_t>(bit) * row_words] = bits[bit];
      }
      return;
   }
   const uint32_t out_bits = map[0] & LAYOUT_ROWS_MASK;  // 2 or 3 code planes, or 0..3 one-hot rows
   const bool one_hot = (map[0] & LAYOUT_ONE_HOT) != 0;
   uint64_t out_plane[3] = {0, 0, 0};
   uint64_t coded = 0;
   if ((map[0] & LAYOUT_IMPLICIT) != 0) {  // the rows of the derived symbol are stored nowhere
      const uint32_t full_code = map[IMPLICIT_SLOT] + 1u;
      uint64_t match = ~0ull;
#pragma unroll
      for (int bit = 0; bit < BITS; ++bit) {
         match &= ((full_code >> bit) & 1u) != 0 ? bits[bit] : ~bits[bit];
      }
      coded |= match;
   }
   for (uint32_t code = 1; code < (one_hot ? out_bits + 1u : (1u << out_bits)); ++code) {
      const uint32_t symbol = map[code];
      if (symbol == 0xFFu) {
         continue;
      }
      const uint32_t full_code = symbol + 1u;
      uint64_t match = ~0ull;
#pragma unroll
      for (int bit = 0; bit < BITS; ++bit) {
         match &= ((full_code >> bit) & 1u) != 0 ? bits[bit] : ~bits[bit];
      }
      coded |= match;
#pragma unroll
      for (uint32_t bit = 0; bit < 3; ++bit) {
         if (one_hot ? code == bit + 1u : ((code >> bit) & 1u) != 0) {
            out_plane[bit] |= match;
         }
      }
   }
   for (uint32_t bit = 0; bit < out_bits; ++bit) {
      out[static_cast<size_t>(bit) * row_words] = out_plane[bit];
   }
   uint64_t escaped = valid & ~coded;
   while (escaped != 0) {
      const uint32_t row_bit = static_cast<uint32_t>(__builtin_ctzll(escaped));
      escaped &= escaped - 1;
      uint32_t full_code = 0;
#pragma unroll
      for (int bit = 0; bit < BITS; ++bit) {
         full_code |= static_cast<uint32_t>((bits[bit] >> row_bit) & 1ull) << bit;
      }
      const size_t counter = static_cast<size_t>(p) * n_scan + (full_code - 1u);
      const uint32_t slot = escape_first[counter] + atomicAdd(escape_cursor + counter, 1u);
      escapes[slot] = (static_cast<uint64_t>(p) << 37) | (static_cast<uint64_t>(full_code - 1u) << 32) | (static_cast<uint64_t>(w) * 64u + row_bit);
   }
}

/// Did the encoding pass of a two-pass build fill every (position, symbol) slice of the key list exactly?
__global__ void k_check_cursors(const uint32_t* __restrict__ first, const uint32_t* __restrict__ cursor, uint32_t n_counters, uint32_t* __restrict__ mismatches) {
   const uint32_t counter = blockIdx.x * blockDim.x + threadIdx.x;
   if (counter < n_counters && cursor[counter] != first[counter + 1] - first[counter]) {
      atomicAdd(mismatches, 1u);
   }
}

/// Every position of the store keeps its n_bits identity planes, where they are (short rows, re-encoding switched off, or no room).
int keepBuildPlanes(SeqStoreHost& seqstore) {
   SeqStoreDev& dev = seqstore.dev;
   seqstore.layout.runs.assign(1, SeqStoreHost::Run{0, dev.positions, static_cast<uint8_t>(dev.n_bits), true, false});
   dev.planes = dev.scan;
   dev.row_of = nullptr;
   dev.code_map = nullptr;
   dev.escapes = nullptr;
   dev.escape_first = nullptr;
   seqstore.layout.built = true;
   return SILO_GPU_OK;
}

/// Does every row of the store have a symbol at every position — a valid one (the totals), the missing one (its runs) or a
/// sparsely stored one (the sorted keys)?  Rows that never received a sequence, or an import whose bitmaps leave rows out,
/// do not; such a store derives nothing (the derived symbol would take them in).
int everyRowHasASymbol(const silo_gpu_store* store, const SeqStoreHost& seqstore, bool* complete) {
   const SeqStoreDev& dev = seqstore.dev;
   const uint32_t positions = dev.positions;
   *complete = false;
   if (seqstore.d_totals.get() == nullptr || !seqstore.totals_ready || dev.kind[dev.missing_symbol] != PLANE_RUNS) {
      return SILO_GPU_OK;
   }
   std::vector<uint32_t> totals, without;
   if (const int rc = downloadTotals(seqstore, totals); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = rowsWithoutSymbol(seqstore, without); rc != SILO_GPU_OK) {
      return rc;
   }
   for (uint32_t p = 0; p < positions; ++p) {
      uint64_t covered = without[p];
      for (uint32_t symbol = 0; symbol < dev.n_scan; ++symbol) {
         covered += totals[static_cast<size_t>(p) * dev.n_scan + symbol];
      }
      if (covered != store->sequence_count) {
         return SILO_GPU_OK;
      }
   }
   *complete = true;
   return SILO_GPU_OK;
}

}  // namespace

namespace silo_gpu_detail {

/// Is this a store finalize re-encodes (5 nucleotide / 22 amino-acid scan symbols, rows of at least one column tile)?
bool reencodes(const silo_gpu_store* store, const SeqStoreDev& dev) {
   const bool nucleotide = dev.n_bits == 3 && dev.n_scan == 5;
   return (nucleotide || (dev.n_bits == 5 && dev.n_scan == 22)) && dev.row_words >= SCAN_THREADS * 4 && dev.positions != 0 && store->sequence_count != 0 &&
          layoutOption(store) >= 0;
}

/// From the totals of the store (seqstore.d_totals): the layout of every position, the tables that describe it and the device
/// arrays of the finished store — the plane rows zeroed when `zero_planes` (an encoder that only sets bits).  *fits = false
/// (nothing allocated) when no position would be re-encoded or the arrays do not fit.
int planLayout(const silo_gpu_store* store, SeqStoreHost& seqstore, SeqStoreHost::LayoutWork& work, bool zero_planes, bool allow_implicit, bool* fits) {
   SeqStoreDev& dev = seqstore.dev;
   const uint32_t positions = dev.positions;
   const size_t n_counters = static_cast<size_t>(positions) * dev.n_scan;
   *fits = false;
   std::vector<uint32_t> totals;
   if (const int rc = downloadTotals(seqstore, totals); rc != SILO_GPU_OK) {
      return rc;
   }
   std::vector<uint32_t> counts;  // escape keys per (position, symbol)
   // SILO_GPU_TUNE_COMPACT_INDEX 2: code planes only, no one-hot rows; 3: one-hot rows with a row for the most numerous symbol
   // too (the layouts of round 2, for comparisons).  The most numerous symbol of a position is derived (LAYOUT_IMPLICIT) only where
   // the rows without a valid symbol can be counted without a plane: the missing symbol kept as runs.
   const int tuned = layoutOption(store);
   const int one_hot_mode = tuned == 2 ? silo_gpu_layout::ONE_HOT_OFF : (tuned == 3 || !allow_implicit ? silo_gpu_layout::ONE_HOT_ROWS : silo_gpu_layout::ONE_HOT_IMPLICIT);
   silo_gpu_layout::chooseLayouts(
      totals, dev.n_scan, dev.n_bits, positions, static_cast<uint64_t>(dev.row_words) * sizeof(uint64_t), one_hot_mode,
      keyCostOption(store) > 0 ? static_cast<uint64_t>(keyCostOption(store)) : KEY_COST_BYTES, work.code_map, counts,
      launchCostOption(store) == 0 ? silo_gpu_layout::LAUNCH_COST_BYTES : (launchCostOption(store) < 0 ? 0 : static_cast<uint64_t>(launchCostOption(store)) << 10)
   );
   work.row_of.assign(positions + 1, 0);
   work.escape_first.assign(positions + 1, 0);
   work.escape_first_symbol.assign(n_counters + 1, 0);
   bool any_encoded = false;
   for (uint32_t p = 0; p < positions; ++p) {
      const uint8_t* map = work.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE;
      const uint8_t bits = map[0] & LAYOUT_ROWS_MASK;
      const bool identity = (map[0] & LAYOUT_IDENTITY) != 0;
      const bool one_hot = (map[0] & LAYOUT_ONE_HOT) != 0;
      any_encoded = any_encoded || !identity;
      work.has_implicit = work.has_implicit || (map[0] & LAYOUT_IMPLICIT) != 0;
      work.row_of[p] = static_cast<uint32_t>(work.total_rows);
      work.total_rows += bits;
      for (uint32_t row = 0; row < bits; ++row) {  // a row without a symbol (no valid symbol at the position at all) is empty: any counter of the position
         work.row_target.push_back(one_hot ? p * dev.n_scan + (map[1 + row] != 0xFFu ? map[1 + row] : 0u) : 0xFFFFFFFFu);
      }
      work.escape_first[p] = static_cast<uint32_t>(work.total_escapes);
      for (uint32_t symbol = 0; symbol < dev.n_scan; ++symbol) {
         work.escape_first_symbol[static_cast<size_t>(p) * dev.n_scan + symbol] = static_cast<uint32_t>(work.total_escapes);
         work.total_escapes += counts[static_cast<size_t>(p) * dev.n_scan + symbol];
      }
      const uint8_t run_bits = one_hot ? 0 : bits;
      if (work.runs.empty() || work.runs.back().bits != run_bits || work.runs.back().identity != identity || work.runs.back().one_hot != one_hot) {
         work.runs.push_back(SeqStoreHost::Run{p, p + 1, run_bits, identity, one_hot});
      } else {
         work.runs.back().end = p + 1;
      }
   }
   work.row_of[positions] = static_cast<uint32_t>(work.total_rows);
   work.escape_first[positions] = static_cast<uint32_t>(work.total_escapes);
   work.escape_first_symbol[n_counters] = static_cast<uint32_t>(work.total_escapes);
   work.plane_bytes = static_cast<size_t>(work.total_rows) * dev.row_words * sizeof(uint64_t);
   work.escape_bytes = std::max<uint64_t>(work.total_escapes, 1) * sizeof(uint64_t);
   size_t free_bytes = 0, total_bytes = 0;
   HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
   // the sort of the keys needs as much again as the keys, their slice-major copy as well
   if (!any_encoded || work.total_rows >= (uint64_t{1} << 32) || work.total_escapes >= (uint64_t{1} << 32) ||
       free_bytes < work.plane_bytes + 4 * work.escape_bytes + (size_t{1} << 30)) {
      work = SeqStoreHost::LayoutWork{};
      return SILO_GPU_OK;
   }
   const size_t plane_words = std::max<size_t>(work.plane_bytes, 256) / sizeof(uint64_t);
   HIP_TRY(work.d_code_map.alloc(work.code_map.size()));
   HIP_TRY(work.d_cursor.alloc(n_counters));
   HIP_TRY(work.d_planes.alloc(plane_words));
   HIP_TRY(work.d_escapes.alloc(work.escape_bytes / sizeof(uint64_t)));
   HIP_TRY(work.d_first.alloc(work.escape_first_symbol.size()));
   HIP_TRY(work.d_row_of.alloc(work.row_of.size()));
   HIP_TRY(work.d_escape_first.alloc(work.escape_first.size()));
   HIP_TRY(work.d_row_target.alloc(std::max<size_t>(work.row_target.size(), 1)));
   HIP_TRY(hipMemcpy(work.d_code_map.get(), work.code_map.data(), work.code_map.size(), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(work.d_first.get(), work.escape_first_symbol.data(), work.escape_first_symbol.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(work.d_row_of.get(), work.row_of.data(), work.row_of.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(work.d_row_target.get(), work.row_target.data(), work.row_target.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(work.d_escape_first.get(), work.escape_first.data(), work.escape_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
   HIP_TRY(hipMemset(work.d_cursor.get(), 0, n_counters * sizeof(uint32_t)));
   if (zero_planes) {  // the encoding pass of a two-pass build only sets bits and fills key slots: a slot it misses must not look like a key
      HIP_TRY(hipMemset(work.d_planes.get(), 0, plane_words * sizeof(uint64_t)));
      HIP_TRY(hipMemset(work.d_escapes.get(), 0xFF, work.escape_bytes));
   }
   HIP_TRY(hipStreamSynchronize(nullptr));  // the fills are only enqueued (null stream)
   *fits = true;
   return SILO_GPU_OK;
}

namespace {

/// The planned layout becomes the store: the keys are sorted (and copied slice-major for the scan's escape pass), the
/// encoders' tables and any build-time planes are released, the device description switches to the adaptive planes.
int finishLayout(silo_gpu_store* store, SeqStoreHost& seqstore, SeqStoreHost::LayoutWork& work) {
   SeqStoreDev& dev = seqstore.dev;
   SeqStoreHost::Layout& layout = seqstore.layout;
   const uint32_t positions = dev.positions;
   if (const int rc = silo_gpu_internal_sort_keys(work.d_escapes.get(), work.total_escapes); rc != SILO_GPU_OK) {  // ascending: (position, symbol, sequence)
      return rc;
   }
   // the slice-major copy of the keys for the scan's escape pass — packed to 4 bytes per key — and where each position's keys
   // begin in every slice
   SliceMajorKeys& sliced = layout.escapes_sliced;
   const uint32_t n_slices = sliceCount(store->sequence_count);
   if (work.total_escapes > 0 && n_slices <= ESCAPE_MAX_SLICES) {
      DeviceArray<uint64_t> d_sorted;  // the keys slice-major, 8 bytes wide: what the packed list is made from
      HIP_TRY(d_sorted.alloc(work.escape_bytes / sizeof(uint64_t)));
      HIP_TRY(hipMemcpy(d_sorted.get(), work.d_escapes.get(), work.total_escapes * sizeof(uint64_t), hipMemcpyDeviceToDevice));
      if (const int rc = packSliceMajor(d_sorted.get(), work.total_escapes, dev.n_scan, positions, n_slices, 0, sliced); rc != SILO_GPU_OK) {
         return rc;
      }
   }
   work.d_first.reset();
   work.d_cursor.reset();
   if (dev.scan != nullptr) {  // the adaptive planes take over; the build-time planes go
      const size_t build_bytes = static_cast<size_t>(positions) * dev.n_bits * dev.row_words * sizeof(uint64_t);
      seqstore.d_scan.reset();
      dev.scan = nullptr;
      store->device_bytes -= build_bytes;
      std::vector<uint8_t>().swap(seqstore.imported_positions);
   }
   layout.planes = std::move(work.d_planes);
   layout.d_row_of = std::move(work.d_row_of);
   layout.d_row_target = std::move(work.d_row_target);
   layout.d_code_map = std::move(work.d_code_map);
   layout.d_escapes = std::move(work.d_escapes);
   layout.slice_shift = ESCAPE_SLICE_SHIFT;
   layout.d_escape_first = std::move(work.d_escape_first);
   layout.row_of = std::move(work.row_of);
   layout.code_map = std::move(work.code_map);
   layout.escape_first = std::move(work.escape_first);
   layout.escape_first_symbol = std::move(work.escape_first_symbol);
   layout.runs = std::move(work.runs);
   layout.has_implicit = work.has_implicit;
   layout.device_bytes = work.plane_bytes + work.escape_bytes + sliced.packed_keys * sizeof(uint32_t) + static_cast<size_t>(sliced.n_overflow) * sizeof(uint64_t) +
                         static_cast<size_t>(positions) * (CODE_MAP_STRIDE + 8) +
                         work.total_rows * sizeof(uint32_t);
   store->device_bytes += layout.device_bytes;
   dev.planes = layout.planes.get();
   dev.row_of = layout.d_row_of.get();
   dev.code_map = layout.d_code_map.get();
   dev.escapes = layout.d_escapes.get();
   dev.escape_first = layout.d_escape_first.get();
   layout.built = true;
   return SILO_GPU_OK;  // (what `work` still owns goes with it: everything else is the store's now)
}

}  // namespace

/// finalize(): derive the adaptive planes of one sequence store from its build-time planes and release those — or keep them as
/// they are when re-encoding would not pay (short rows), is switched off (SILO_GPU_TUNE_COMPACT_INDEX < 0) or does not fit
/// next to them.  A store built in two passes has been encoded already: only the keys remain to be put in order.
int buildLayout(silo_gpu_store* store, SeqStoreHost& seqstore) {
   SeqStoreDev& dev = seqstore.dev;
   SeqStoreHost::Layout& layout = seqstore.layout;
   const uint32_t positions = dev.positions;
   if (dev.build_mode == BUILD_ENCODE) {
      HIP_TRY(hipDeviceSynchronize());
      dev.build_mode = BUILD_PLANES;
      const std::shared_ptr<SeqStoreHost::LayoutWork> work = std::move(seqstore.work);  // freed on every way out
      {  // every (position, symbol) must have received exactly the keys the first pass counted for it
         const uint32_t n_counters = positions * dev.n_scan;
         DeviceArray<uint32_t> d_mismatch;
         uint32_t mismatch = 0;
         HIP_TRY(d_mismatch.alloc(1));
         hipError_t status = hipMemset(d_mismatch.get(), 0, sizeof(uint32_t));
         if (status == hipSuccess && n_counters != 0) {
            k_check_cursors<<<(n_counters + 255) / 256, 256>>>(work->d_first.get(), work->d_cursor.get(), n_counters, d_mismatch.get());
            status = hipGetLastError();
         }
         status = status != hipSuccess ? status : hipMemcpy(&mismatch, d_mismatch.get(), sizeof(uint32_t), hipMemcpyDeviceToHost);
         d_mismatch.reset();
         if (status != hipSuccess || mismatch != 0) {
            HIP_TRY(status);
            return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "two-pass build: the second pass did not bring the rows the first pass counted (escape keys of " + std::to_string(mismatch) + " (position, symbol) cells differ)");
         }
      }
      if (work->has_implicit) {
         bool complete = false;
         if (const int rc = everyRowHasASymbol(store, seqstore, &complete); rc != SILO_GPU_OK) {
            return rc;
         }
         if (!complete) {
            return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "two-pass build: some row of the store has no symbol at some position (every row has to be filled in both passes)");
         }
      }
      return finishLayout(store, seqstore, *work);
   }
   if (!reencodes(store, dev)) {
      return keepBuildPlanes(seqstore);
   }
   // the unfiltered totals decide the codes (and are what a full filter adds later on)
   const size_t n_counters = static_cast<size_t>(positions) * dev.n_scan;
   if (seqstore.d_totals.get() == nullptr) {
      HIP_TRY(seqstore.d_totals.alloc(n_counters));
   }
   if (!seqstore.totals_ready) {
      HIP_TRY(hipMemsetAsync(seqstore.d_totals.get(), 0, n_counters * sizeof(uint32_t), nullptr));
      ScanRange all{&seqstore, 0, positions, {}};
      all.counts[0] = seqstore.d_totals.get();
      const uint64_t* ones = store->d_ones.get();
      layout.runs.clear();  // scan the build-time planes
      const int rc = scanRanges(store, {all}, &ones, 1, nullptr);
      if (rc != SILO_GPU_OK) {
         return rc;
      }
      HIP_TRY(hipStreamSynchronize(nullptr));
      seqstore.totals_ready = true;
   }
   SeqStoreHost::LayoutWork work;
   bool fits = false;
   bool complete = false;  // only a store whose every row has a symbol at every position may derive one as "the rest"
   if (dev.kind[dev.missing_symbol] == PLANE_RUNS) {
      if (const int rc = everyRowHasASymbol(store, seqstore, &complete); rc != SILO_GPU_OK) {
         return rc;
      }
   }
   if (const int rc = planLayout(store, seqstore, work, false, complete, &fits); rc != SILO_GPU_OK) {
      return rc;
   }
   if (!fits) {
      return keepBuildPlanes(seqstore);
   }
   {
      const dim3 grid((dev.row_words + 255) / 256, positions);
      const auto encode = dev.n_bits == 3 ? k_encode_adaptive<3> : k_encode_adaptive<5>;
      encode<<<grid, 256>>>(
         dev.scan, dev.row_words, dev.n_scan, work.d_code_map.get(), work.d_row_of.get(), work.d_first.get(), work.d_cursor.get(), work.d_planes.get(),
         work.d_escapes.get()
      );
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
   }
   if (const int rc = walkEndRuns(store, seqstore, work.has_implicit); rc != SILO_GPU_OK) {  // (the build-time planes go in finishLayout)
      return rc;
   }
   return finishLayout(store, seqstore, work);
}

}  // namespace silo_gpu_detail
