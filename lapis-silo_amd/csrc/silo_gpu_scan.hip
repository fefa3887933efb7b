// silo_gpu_scan.hip — K1, the Mutations scan of the SILO mutation-filter hot path on CDNA4 (gfx950): the scan over ranges (DESIGN.md
// §3, "K1 design" to "K1c / batched queries"; "Host side").  The passes and their kernels live in files of their own
// (scan_internal.h); here is what ties them together: the ranges cut into pieces by layout, the timing log, the pool of
// scratch blocks, the side streams, the order of the passes; and the C entries silo_gpu_mutations_scan*, silo_gpu_scan_timings,
// silo_gpu_last_scan_kernel, silo_gpu_last_escape_items and the silo_gpu_store_scan_* statistics.
//
// Kernels:
//   k_add_u32   the cached totals of the unfiltered store added to a count table (silo_gpu_mutations_scan without a filter)
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fused_select_rule.h"
#include "scan_internal.h"

using namespace silo_gpu_detail;

namespace {

thread_local const char* g_last_scan_kernel = "none";

__global__ void k_add_u32(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n) {
   const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) {
      dst[i] += src[i];
   }
}

ScanLayout layoutOfRun(const SeqStoreDev& dev, uint32_t bits, bool identity, bool one_hot) {
   if (one_hot) {
      return SCAN_ONE_HOT_ROWS;
   }
   if (!identity) {
      return bits == 2 ? SCAN_2_PLANES : SCAN_3_PLANES_MAPPED;
   }
   return dev.n_bits == 3 ? SCAN_FULL_NUCLEOTIDE : SCAN_FULL_AMINO_ACID;
}

/// Cuts the ranges along the runs of their stores; pieces[layout] collects what one kind of launch takes.  end_runs (or nullptr):
/// per range, whether the scan counts the end runs of the gap symbol there (DerivedPlan::end_runs) — its runs of one-hot rows
/// then carry the flags of the rows to leave out.
void cutIntoPieces(const std::vector<ScanRange>& ranges, uint32_t q_count, std::vector<ScanPiece> (&pieces)[N_SCAN_LAYOUTS], const std::vector<uint8_t>* end_runs) {
   for (const ScanRange& range : ranges) {
      const bool covered = end_runs != nullptr && (*end_runs)[static_cast<size_t>(&range - ranges.data())] != 0;
      const SeqStoreHost& seqstore = *range.seqstore;
      const SeqStoreDev& dev = seqstore.dev;
      const auto add = [&](uint32_t begin, uint32_t end, uint32_t bits, bool identity, bool one_hot) {
         begin = std::max(begin, range.pos_begin);
         end = std::min(end, range.pos_end);
         if (begin >= end) {
            return;
         }
         ScanPiece piece{};
         const bool encoded = seqstore.layout.built && seqstore.layout.d_row_of.get() != nullptr;
         const size_t first_row = encoded ? seqstore.layout.row_of[begin] : static_cast<size_t>(begin) * dev.n_bits;
         piece.planes = dev.planes + first_row * dev.row_words;
         piece.n_positions = end - begin;
         if (one_hot) {
            piece.code_map = reinterpret_cast<const uint8_t*>(seqstore.layout.d_row_target.get() + first_row);
            piece.n_positions = seqstore.layout.row_of[end] - seqstore.layout.row_of[begin];
            piece.target_base = begin * dev.n_scan;
            if (seqstore.layout.d_row_heaviest.get() != nullptr && seqstore.layout.d_row_without.get() != nullptr) {
               piece.row_heaviest = seqstore.layout.d_row_heaviest.get() + first_row;
               piece.row_without = seqstore.layout.d_row_without.get() + first_row;
            }
            piece.row_covered = covered ? seqstore.layout.d_row_covered.get() + first_row : nullptr;
            if (piece.n_positions == 0) {
               return;  // positions whose only stored symbol is derived: no rows
            }
         } else if (!identity) {
            piece.code_map = seqstore.layout.d_code_map.get() + static_cast<size_t>(begin) * CODE_MAP_STRIDE;
         }
         for (uint32_t q = 0; q < q_count; ++q) {
            piece.counts[q] = range.counts[q] + static_cast<size_t>(begin - range.pos_begin) * dev.n_scan;
         }
         pieces[layoutOfRun(dev, bits, identity, one_hot)].push_back(piece);
      };
      if (seqstore.layout.runs.empty()) {  // still the build-time planes (the totals scan inside finalize)
         add(0, dev.positions, dev.n_bits, true, false);
      }
      for (const SeqStoreHost::Run& run : seqstore.layout.runs) {
         add(run.begin, run.end, run.bits, run.identity, run.one_hot);
      }
   }
}

}  // namespace

namespace silo_gpu_detail {

/// Event pairs around the plane-scan launches of this thread's last scan (SILO_GPU_TUNE_SCAN_TIMING); the events are
/// created once and reused.
struct ScanLaunchTiming {
   hipEvent_t start = nullptr;
   hipEvent_t stop = nullptr;
   silo_gpu_scan_timing entry{};
};
struct ScanTimingLog {
   std::vector<ScanLaunchTiming> launches;
   size_t used = 0;
};
static ScanTimingLog& scanTimingLog() {
   thread_local ScanTimingLog log;
   return log;
}

/// With SILO_GPU_TUNE_SCAN_TIMING set: an entry of the thread's timing log with its start event recorded on `stream` (the
/// stream the launch that follows goes to); nullptr otherwise.  `bytes` = what the launch has to read, each byte once.
ScanLaunchTiming* startLaunchTiming(const char* kernel, uint64_t plane_rows, uint64_t bytes, uint32_t filters, uint32_t blocks, hipStream_t stream) {
   if (g_tune_scan_timing.load() != 1) {
      return nullptr;
   }
   ScanTimingLog& log = scanTimingLog();
   if (log.used == log.launches.size()) {
      ScanLaunchTiming fresh;
      if (hipEventCreate(&fresh.start) != hipSuccess || hipEventCreate(&fresh.stop) != hipSuccess) {
         (void)hipGetLastError();
         return nullptr;
      }
      log.launches.push_back(fresh);
   }
   ScanLaunchTiming* timing = &log.launches[log.used++];
   std::snprintf(timing->entry.kernel, sizeof(timing->entry.kernel), "%s", kernel);
   timing->entry.plane_rows = plane_rows;
   timing->entry.bytes = bytes;
   timing->entry.filters = filters;
   timing->entry.blocks = blocks;
   if (hipEventRecord(timing->start, stream) != hipSuccess) {
      (void)hipGetLastError();
      --log.used;
      return nullptr;
   }
   return timing;
}

void finishLaunchTiming(ScanLaunchTiming* timing, hipStream_t stream) {
   if (timing != nullptr) {
      (void)hipEventRecord(timing->stop, stream);
   }
}

}  // namespace silo_gpu_detail

namespace {

/// Device scratch of a scan: per filter the counters of the prepare step (TWO sets: a scan uses one and zeroes the other for
/// the next scan on this block, so no fill launch is needed), the list of sector indexes of the sparse-filter routing, and
/// the private tables of a scan with derived symbols.  Blocks are pooled; a block is handed out again only once the event
/// recorded after its last use has completed, whatever stream that use was on.
struct SparseScratch {
   int device = 0;
   uint32_t capacity = 0;  // sectors per filter
   uint32_t* counters[2] = {nullptr, nullptr};  // [SILO_GPU_MAX_SCAN_BATCH * SPARSE_COUNTER_STRIDE] each
   uint32_t set = 0;                            // the counter set of the current use
   uint32_t* sector_index = nullptr;            // [SILO_GPU_MAX_SCAN_BATCH][capacity]
   uint32_t* tables = nullptr;                  // private count tables (scans with derived symbols)
   size_t table_words = 0;
   hipEvent_t last_use = nullptr;
   bool in_flight = false;  // handed out and not yet released
};

std::mutex g_sparse_scratch_mutex;
std::vector<SparseScratch*> g_sparse_scratch;

int acquireSparseScratch(int device, uint32_t capacity, size_t table_words, SparseScratch** out) {
   {
      std::lock_guard<std::mutex> lock(g_sparse_scratch_mutex);
      for (SparseScratch* block : g_sparse_scratch) {
         if (!block->in_flight && block->device == device && block->capacity >= capacity && block->table_words >= table_words &&
             hipEventQuery(block->last_use) == hipSuccess) {
            block->in_flight = true;
            block->set ^= 1u;
            *out = block;
            return SILO_GPU_OK;
         }
      }
   }
   auto block = std::make_unique<SparseScratch>();
   block->device = device;
   block->capacity = capacity;
   block->table_words = std::max<size_t>(table_words, size_t{1} << 20);
   void* memory = nullptr;  // raw on purpose: the pool lives as long as the process and is never freed (the HIP runtime may be gone by then)
   // one allocation: the private tables, the index lists, then the two counter sets (zeroed here, by the scans from then on)
   const size_t counter_words = static_cast<size_t>(SILO_GPU_MAX_SCAN_BATCH) * SPARSE_COUNTER_STRIDE;
   const size_t bytes = (block->table_words + static_cast<size_t>(SILO_GPU_MAX_SCAN_BATCH) * capacity + 2 * counter_words) * sizeof(uint32_t);
   HIP_TRY(hipMalloc(&memory, bytes));
   block->tables = static_cast<uint32_t*>(memory);
   block->sector_index = block->tables + block->table_words;
   block->counters[0] = block->sector_index + static_cast<size_t>(SILO_GPU_MAX_SCAN_BATCH) * capacity;
   block->counters[1] = block->counters[0] + counter_words;
   hipError_t status = hipMemset(block->counters[0], 0, 2 * counter_words * sizeof(uint32_t));
   status = status != hipSuccess ? status : hipStreamSynchronize(nullptr);  // the fill is only enqueued; the scans run on other streams
   status = status != hipSuccess ? status : hipEventCreateWithFlags(&block->last_use, hipEventDisableTiming);
   if (status != hipSuccess) {
      (void)hipFree(memory);
      return fail(SILO_GPU_ERR_HIP, "scan scratch: " + std::string(hipGetErrorString(status)));
   }
   block->in_flight = true;
   std::lock_guard<std::mutex> lock(g_sparse_scratch_mutex);
   g_sparse_scratch.push_back(block.get());
   *out = block.release();
   return SILO_GPU_OK;
}

void releaseSparseScratch(SparseScratch* block, hipStream_t stream) {
   (void)hipEventRecord(block->last_use, stream);
   std::lock_guard<std::mutex> lock(g_sparse_scratch_mutex);
   block->in_flight = false;
}



/// Side streams (and the events that tie them to the caller's) per host thread.  The escape pass is a stream of keys, random
/// filter lookups and atomics — latency-bound — and adds to the same count tables as the plane scans, which are
/// bandwidth-bound, so it runs beside them.  Never destroyed (thread exit may come after the HIP runtime has shut down).
constexpr int N_SIDE_STREAMS = 2;  // the escape pass: [0] at the lowest stream priority, [1] at the default one (SILO_GPU_TUNE_SIDE_STREAM)
struct SideStreams {
   hipStream_t stream[N_SIDE_STREAMS] = {nullptr, nullptr};
   hipEvent_t fork[2] = {nullptr, nullptr};
   hipEvent_t join[N_SIDE_STREAMS] = {nullptr, nullptr};
   bool used[N_SIDE_STREAMS] = {false, false};
   bool tried = false;
   bool ok = false;
};

SideStreams* sideStreams() {
   thread_local SideStreams side;
   if (!side.tried) {
      side.tried = true;
      side.ok = true;
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      for (int k = 0; k < N_SIDE_STREAMS; ++k) {
         side.ok = side.ok && hipStreamCreateWithPriority(&side.stream[k], hipStreamNonBlocking, k == 0 ? least : 0) == hipSuccess &&
                   hipEventCreateWithFlags(&side.join[k], hipEventDisableTiming) == hipSuccess;
      }
      for (int k = 0; k < 2; ++k) {
         side.ok = side.ok && hipEventCreateWithFlags(&side.fork[k], hipEventDisableTiming) == hipSuccess;
      }
      if (!side.ok) {
         (void)hipGetLastError();
      }
   }
   return side.ok ? &side : nullptr;
}

/// Makes side stream `k` wait for everything queued on `hip_stream` so far (through fork event `fork_index`).
int forkSide(SideStreams* side, int k, int fork_index, hipStream_t hip_stream, bool record) {
   if (record) {
      HIP_TRY(hipEventRecord(side->fork[fork_index], hip_stream));
   }
   HIP_TRY(hipStreamWaitEvent(side->stream[k], side->fork[fork_index], 0));
   side->used[k] = true;
   return SILO_GPU_OK;
}

/// Makes `hip_stream` wait for every side stream that was used since the last join.
int joinSides(hipStream_t hip_stream) {
   SideStreams* side = sideStreams();
   if (side == nullptr) {
      return SILO_GPU_OK;
   }
   for (int k = 0; k < N_SIDE_STREAMS; ++k) {
      if (side->used[k]) {
         side->used[k] = false;
         HIP_TRY(hipEventRecord(side->join[k], side->stream[k]));
         HIP_TRY(hipStreamWaitEvent(hip_stream, side->join[k], 0));
      }
   }
   return SILO_GPU_OK;
}

/// The passes beside the plane scans.  A store with a row for every stored symbol: the escape keys on side stream 0 (lowest
/// priority), beside plane scans that take milliseconds.  A scan with derived symbols has few plane rows left and its escape
/// pass is as long as its plane scans — both stream at the memory's rate and gain nothing from sharing it —, so the escape
/// pass stays on the caller's stream in front of the plane scans, and the side stream (default priority) takes the passes
/// that are bound by latency and LDS, not by bandwidth: the runs of the missing symbol and the sparse keys.  Forked behind
/// everything already queued on `hip_stream` (the filters are complete, the tables zeroed), joined by joinSides before
/// anything reads the tables.  SILO_GPU_TUNE_SIDE_STREAM: 0 as described, 1 side stream of default priority, 2 everything on the caller's stream.
int forkSidePasses(
   const std::vector<ScanRange>& ranges, const uint64_t* const* filters, uint32_t q_count, DerivedPlan* derived, hipStream_t hip_stream,
   const ScanPruning* pruning
) {
   bool any_escapes = false;
   for (const ScanRange& range : ranges) {
      const SeqStoreHost::Layout& layout = range.seqstore->layout;
      any_escapes = any_escapes || (layout.built && layout.d_escapes.get() != nullptr && layout.escape_first[range.pos_end] != layout.escape_first[range.pos_begin]);
   }
   if (!any_escapes && derived == nullptr) {
      return SILO_GPU_OK;
   }
   if (derived != nullptr && derived->events) {  // one pass over the keys, the gap events and the end events, on the caller's stream
      // (SILO_GPU_TUNE_END_RUNS = 1: the end events in a launch of their own behind the row launch — scanRanges; measured, not faster)
      return scanEscapes(ranges, filters, q_count, hip_stream, &derived->gap_ranges, pruning, derived->ends_apart ? nullptr : &derived->end_ranges);
   }
   const int mode = g_tune_side_stream.load();
   SideStreams* side = mode == 2 ? nullptr : sideStreams();
   hipStream_t stream = hip_stream;
   if (side != nullptr) {
      const int k = mode == 1 || derived != nullptr ? 1 : 0;
      if (const int rc = forkSide(side, k, 0, hip_stream, true); rc != SILO_GPU_OK) {
         return rc;
      }
      stream = side->stream[k];
   }
   if (derived != nullptr) {
      if (const int rc = scanRowsWithoutSymbol(*derived, q_count, stream); rc != SILO_GPU_OK) {
         return rc;
      }
      return any_escapes ? scanEscapes(ranges, filters, q_count, mode == 1 ? stream : hip_stream, nullptr, nullptr) : SILO_GPU_OK;
   }
   return scanEscapes(ranges, filters, q_count, stream, nullptr, nullptr);
}

}  // namespace

/// Scan of up to SILO_GPU_MAX_SCAN_BATCH filters over position ranges of sequence stores of one alphabet, with the
/// sparse-filter routing (K1s) around the dense kernels: every filter is compacted ONCE for all ranges, the dense
/// kernels skip the sparse ones, the gather kernel serves them.  All decisions are taken on the device.  Where a store
/// derives the most numerous symbol of its positions the kernels count into private tables and k_finish_scan completes them.
/// `min_proportion` (nullptr, or one per filter): see silo_gpu_mutations_scan_ranges_min_proportion.
int silo_gpu_detail::scanRanges(
   const silo_gpu_store* store, const std::vector<ScanRange>& caller_ranges, const uint64_t* const* filters, uint32_t q_count, hipStream_t hip_stream,
   const double* min_proportion, const ScanSelect* select
) {
   const SeqStoreDev& any_store = caller_ranges.front().seqstore->dev;
   const bool nucleotide = any_store.n_bits == 3 && any_store.n_scan == 5;
   if (!nucleotide && !(any_store.n_bits == 5 && any_store.n_scan == 22)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "mutations scan: unsupported set of scan symbols (5 nucleotide or 22 amino-acid symbols)");
   }
   if (any_store.row_words < SCAN_THREADS * 4) {
      if (select != nullptr) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "mutations scan: short rows do not go through the finish kernel");
      }
      const int rc = scanShortRows(caller_ranges, nucleotide, filters, q_count, hip_stream);
      if (rc == SILO_GPU_OK) {
         g_last_scan_kernel = "k_scan_sliced_rowwave";
      }
      return rc;
   }
   g_last_scan_kernel = q_count == 1 ? "k_scan_sliced" : "k_scan_sliced_batch";
   scanTimingLog().used = 0;
   bool any_derived = false;
   for (const ScanRange& range : caller_ranges) {
      any_derived = any_derived || range.seqstore->layout.has_implicit;
   }
   DerivedPlan plan;
   if (any_derived) {
      planDerived(store, caller_ranges, filters, q_count, plan, select);
   }
   if (select != nullptr && !plan.select) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "mutations scan: this scan cannot select its rows in the finish kernel");  // (canFuseSelect decides the same way)
   }
   const int divisor = g_tune_sparse_divisor.load();
   const bool routing = divisor >= 0;
   if (!routing && !any_derived) {
      std::vector<ScanPiece> pieces[N_SCAN_LAYOUTS];
      cutIntoPieces(caller_ranges, q_count, pieces, nullptr);
      int rc = forkSidePasses(caller_ranges, filters, q_count, nullptr, hip_stream, nullptr);
      if (rc == SILO_GPU_OK) {
         rc = scanPiecesDense(pieces, any_store, filters, q_count, nullptr, 0, hip_stream, nullptr);
      }
      const int joined = joinSides(hip_stream);
      return rc != SILO_GPU_OK ? rc : joined;
   }
   const uint32_t capacity = std::max<uint32_t>(4, any_store.row_words / static_cast<uint32_t>(divisor <= 0 ? 16 : divisor));
   SparseScratch* scratch = nullptr;
   const int acquired = acquireSparseScratch(store->device, capacity, plan.table_words + plan.part_words, &scratch);
   if (acquired != SILO_GPU_OK) {
      return acquired;
   }
   const uint32_t stride = scratch->capacity;  // the block may be larger than asked for
   uint32_t* counters = scratch->counters[scratch->set];
   if (any_derived) {
      bindDerived(plan, scratch->tables, counters, q_count);
   }
   const std::vector<ScanRange>& ranges = any_derived ? plan.private_ranges : caller_ranges;
   std::vector<ScanPiece> pieces[N_SCAN_LAYOUTS];
   cutIntoPieces(ranges, q_count, pieces, any_derived ? &plan.end_runs : nullptr);  // (planDerived decided where the end runs are counted)
   // what the passes may leave out (ScanPruning: the one place that decides it)
   bool some_proportion = false;
   for (uint32_t q = 0; min_proportion != nullptr && q < q_count; ++q) {
      some_proportion = some_proportion || (min_proportion[q] > 0 && min_proportion[q] <= 1);
   }
   const int prune_knob = g_tune_prune_keys.load();
   const bool prune_keys = some_proportion && plan.events && prune_knob >= 0;
   const ScanPruning pruning{counters, min_proportion, prune_keys, prune_keys && prune_knob == 0};
   const ScanPruning* pruned = pruning.keys ? &pruning : nullptr;
   // the prepare step, one launch in front of everything else
   if (prepareScan(filters, q_count, any_store.row_words, stride, counters, scratch->sector_index, scratch->tables, static_cast<uint32_t>(plan.table_words),
                   scratch->counters[scratch->set ^ 1u], hip_stream) != hipSuccess) {
      scratch->set ^= 1u;  // the other set was not re-armed: the next use takes this one again
      releaseSparseScratch(scratch, hip_stream);
      return fail(SILO_GPU_ERR_HIP, "mutations scan: the prepare step could not be launched");
   }
   // the side passes are forked behind the prepare step: the plane scans wait for its counters, and beside a launch that
   // fills the device it takes ten times as long (62 instead of 6 us)
   int rc = forkSidePasses(ranges, filters, q_count, any_derived ? &plan : nullptr, hip_stream, pruned);
   if (rc == SILO_GPU_OK) {
      // (the rows are left out where the keys are: one pass over keys and gap events, the tables completed by k_finish_scan)
      rc = scanPiecesDense(pieces, any_store, filters, q_count, routing ? counters : nullptr, capacity, hip_stream, pruned);
   }
   if (rc == SILO_GPU_OK && any_derived && plan.events && plan.ends_apart) {
      rc = scanEscapes(ranges, filters, q_count, hip_stream, &plan.gap_ranges, nullptr, &plan.end_ranges, true);
   }
   if (rc == SILO_GPU_OK && routing) {
      rc = scanPiecesGather(pieces, any_store, filters, q_count, counters, capacity, scratch->sector_index, stride, hip_stream);
   }
   const int joined = joinSides(hip_stream);  // before the scratch is released: side-stream scans read its counters
   if (rc == SILO_GPU_OK && joined == SILO_GPU_OK && any_derived) {
      rc = finishDerived(plan, q_count, hip_stream);
   }
   releaseSparseScratch(scratch, hip_stream);
   return rc != SILO_GPU_OK ? rc : joined;
}

/// May the finish kernel of the scan behind silo_gpu_mutations_scan_select overwrite the sinks' tables and select their rows?
/// (The arguments have passed the entry's checks.)  Every range goes through k_finish_scan<true, .> — one alphabet, rows long
/// enough for k_scan_sliced, a store with derived symbols, gap events counted — and the ranges tile every filter's table, at the
/// same offsets for all filters (DerivedRange::table_offset); table_offset gets them, per range.
static bool canFuseSelect(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, uint32_t n_filters, uint32_t* const* counts_out_dev,
   const silo_gpu_select_sink* sinks, std::vector<uint32_t>& table_offset
) {
   if (g_tune_fused_select.load() < 0 || n_ranges == 0 || n_filters == 0) {
      return false;
   }
   const uint32_t n_symbols = sinks[0].n_symbols;
   if (n_symbols != 5 && n_symbols != 22) {
      return false;
   }
   std::vector<ScanRange> group;
   std::vector<TableSpan> spans;
   bool any_derived = false;
   table_offset.assign(n_ranges, 0);
   for (uint32_t r = 0; r < n_ranges; ++r) {
      const SeqStoreHost& seqstore = store->seqstores[ranges[r].seqstore_id];
      const uint32_t n = ranges[r].pos_end - ranges[r].pos_begin;
      if (n == 0) {
         continue;  // (not scanned)
      }
      if (seqstore.dev.n_scan != n_symbols || seqstore.dev.planes == nullptr || seqstore.dev.row_words < static_cast<uint32_t>(SCAN_THREADS) * 4) {
         return false;
      }
      any_derived = any_derived || seqstore.layout.has_implicit;
      group.push_back(ScanRange{&seqstore, ranges[r].pos_begin, ranges[r].pos_end, {}});
      for (uint32_t q = 0; q < n_filters; ++q) {
         const silo_gpu_select_sink& sink = sinks[q];
         const uint32_t* at = counts_out_dev[static_cast<size_t>(r) * n_filters + q];
         if (sink.n_symbols != n_symbols || sink.total_positions != sinks[0].total_positions || at < sink.table_dev) {
            return false;
         }
         const size_t words = static_cast<size_t>(at - sink.table_dev);
         if (words % n_symbols != 0 || words / n_symbols >= sink.total_positions) {
            return false;
         }
         const auto offset = static_cast<uint32_t>(words / n_symbols);
         if (q != 0 && offset != table_offset[r]) {
            return false;
         }
         table_offset[r] = offset;
      }
      spans.push_back({table_offset[r], n});
   }
   return any_derived && derivedCountsEvents(group) && spansTileTable(spans, sinks[0].total_positions);
}

/// silo_gpu_mutations_scan_ranges, silo_gpu_mutations_scan_ranges_min_proportion and silo_gpu_mutations_scan_select (`entry`: the
/// one called, for its error messages).  sinks (or nullptr), table_offset: the finish kernel overwrites the tables and selects (canFuseSelect).
static int scanRangesEntry(
   const char* entry, const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   const double* min_proportion, uint32_t* const* counts_out_dev, void* stream, const silo_gpu_select_sink* sinks = nullptr,
   const std::vector<uint32_t>* table_offset = nullptr
) {
   if (store == nullptr || (n_ranges != 0 && ranges == nullptr) || (n_filters != 0 && filters_dev == nullptr) ||
       (n_ranges != 0 && n_filters != 0 && counts_out_dev == nullptr)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad arguments");
   }
   for (uint32_t q = 0; q < n_filters; ++q) {
      if (filters_dev[q] == nullptr) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": null filter");
      }
   }
   for (uint32_t r = 0; r < n_ranges; ++r) {
      if (ranges[r].seqstore_id >= store->seqstores.size()) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": no such sequence store");
      }
      const SeqStoreDev& dev = store->seqstores[ranges[r].seqstore_id].dev;
      if (ranges[r].pos_begin > ranges[r].pos_end || ranges[r].pos_end > dev.positions) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "position range out of bounds");
      }
      for (uint32_t q = 0; q < n_filters; ++q) {
         if (counts_out_dev[static_cast<size_t>(r) * n_filters + q] == nullptr) {
            return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": null counts buffer");
         }
      }
   }
   if (n_ranges == 0 || n_filters == 0) {
      return SILO_GPU_OK;
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);
   for (uint32_t first = 0; first < n_filters; first += SILO_GPU_MAX_SCAN_BATCH) {
      const uint32_t q_count = std::min<uint32_t>(SILO_GPU_MAX_SCAN_BATCH, n_filters - first);
      // ranges of one layout (3 code planes / 5 code planes) share launches
      for (const uint32_t n_bits : {3u, 5u}) {
         std::vector<ScanRange> group;
         ScanSelect select;
         for (uint32_t r = 0; r < n_ranges; ++r) {
            const SeqStoreDev& dev = store->seqstores[ranges[r].seqstore_id].dev;
            if (ranges[r].pos_begin == ranges[r].pos_end || dev.n_scan == 0 || (dev.n_bits == 3 ? 3u : 5u) != n_bits) {
               continue;
            }
            const SeqStoreHost& seqstore = store->seqstores[ranges[r].seqstore_id];
            if (dev.planes == nullptr) {
               return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": the sequence store holds no sequences yet");
            }
            ScanRange range{&seqstore, ranges[r].pos_begin, ranges[r].pos_end, {}};
            for (uint32_t q = 0; q < q_count; ++q) {
               range.counts[q] = counts_out_dev[static_cast<size_t>(r) * n_filters + first + q];
            }
            group.push_back(range);
            if (sinks != nullptr) {
               select.table_offset.push_back((*table_offset)[r]);
            }
         }
         for (uint32_t q = 0; sinks != nullptr && !group.empty() && q < q_count; ++q) {  // (one alphabet: one group per filter)
            const silo_gpu_select_sink& sink = sinks[first + q];
            silo_gpu_row_slot* slot = sink.slot;
            slot->epoch += 1;
            if (slot->epoch == 0) {
               slot->epoch = 1;
            }
            select.sinks[q] = SelectSink{
               sink.reference_index_dev, slot->d_cursor_and_ticket.get(), reinterpret_cast<silo_gpu_mutation_row*>(static_cast<char*>(slot->host_dev) + 16),
               static_cast<unsigned long long*>(slot->host_dev), min_proportion != nullptr ? min_proportion[first + q] : 0.0, slot->capacity, slot->epoch, 0};
         }
         if (!group.empty()) {
            const int rc = scanRanges(store, group, filters_dev + first, q_count, hip_stream, min_proportion != nullptr ? min_proportion + first : nullptr,
                                      sinks != nullptr ? &select : nullptr);
            if (rc != SILO_GPU_OK) {
               return rc;
            }
         }
      }
   }
   return SILO_GPU_OK;
}

extern "C" {

const char* silo_gpu_last_scan_kernel(void) {
   return g_last_scan_kernel;
}

uint32_t silo_gpu_last_escape_items(void) {
   return g_last_escape_items;
}

int silo_gpu_mutations_scan_ranges(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   uint32_t* const* counts_out_dev, void* stream
) {
   return scanRangesEntry("silo_gpu_mutations_scan_ranges", store, ranges, n_ranges, filters_dev, n_filters, nullptr, counts_out_dev, stream);
}

int silo_gpu_mutations_scan_ranges_min_proportion(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   const double* min_proportion, uint32_t* const* counts_out_dev, void* stream
) {
   return scanRangesEntry("silo_gpu_mutations_scan_ranges_min_proportion", store, ranges, n_ranges, filters_dev, n_filters, min_proportion, counts_out_dev, stream);
}

int silo_gpu_mutations_scan_select(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   const double* min_proportion, uint32_t* const* counts_out_dev, const silo_gpu_select_sink* sinks, void* stream
) {
   const char* entry = "silo_gpu_mutations_scan_select";
   if (store == nullptr || sinks == nullptr || n_filters == 0 || filters_dev == nullptr || n_ranges == 0 || ranges == nullptr || counts_out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad arguments");
   }
   for (uint32_t q = 0; q < n_filters; ++q) {
      const silo_gpu_select_sink& sink = sinks[q];
      if (filters_dev[q] == nullptr || sink.table_dev == nullptr || sink.reference_index_dev == nullptr || sink.slot == nullptr || sink.total_positions == 0 ||
          sink.n_symbols == 0 || sink.n_symbols > 32) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad filter or sink");
      }
      for (uint32_t other = 0; other < q; ++other) {
         if (sinks[other].slot == sink.slot || sinks[other].table_dev == sink.table_dev) {
            return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": two filters share a table or a row slot");
         }
      }
   }
   // (the checks both routes share come first: a call that fails them has launched nothing)
   for (uint32_t r = 0; r < n_ranges; ++r) {
      if (ranges[r].seqstore_id >= store->seqstores.size()) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": no such sequence store");
      }
      if (ranges[r].pos_begin > ranges[r].pos_end || ranges[r].pos_end > store->seqstores[ranges[r].seqstore_id].dev.positions) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "position range out of bounds");
      }
      for (uint32_t q = 0; q < n_filters; ++q) {
         if (counts_out_dev[static_cast<size_t>(r) * n_filters + q] == nullptr) {
            return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string(entry) + ": null counts buffer");
         }
      }
   }
   std::vector<uint32_t> table_offset;
   if (canFuseSelect(store, ranges, n_ranges, n_filters, counts_out_dev, sinks, table_offset)) {
      return scanRangesEntry(entry, store, ranges, n_ranges, filters_dev, n_filters, min_proportion, counts_out_dev, stream, sinks, &table_offset);
   }
   // otherwise what a caller of the other entries does: clear the tables, scan into them, select from them (K4)
   HIP_TRY(hipSetDevice(store->device));
   for (uint32_t q = 0; q < n_filters; ++q) {
      HIP_TRY(hipMemsetAsync(sinks[q].table_dev, 0, static_cast<size_t>(sinks[q].total_positions) * sinks[q].n_symbols * sizeof(uint32_t), static_cast<hipStream_t>(stream)));
   }
   if (const int rc = scanRangesEntry(entry, store, ranges, n_ranges, filters_dev, n_filters, min_proportion, counts_out_dev, stream); rc != SILO_GPU_OK) {
      return rc;
   }
   for (uint32_t q = 0; q < n_filters; ++q) {
      const int rc = silo_gpu_mutations_select_to_slot(
         sinks[q].table_dev, sinks[q].reference_index_dev, sinks[q].total_positions, sinks[q].n_symbols, min_proportion != nullptr ? min_proportion[q] : 0.0,
         sinks[q].slot, stream
      );
      if (rc != SILO_GPU_OK) {
         return rc;
      }
   }
   return SILO_GPU_OK;
}

int silo_gpu_scan_timings(silo_gpu_scan_timing* out, uint32_t capacity, uint32_t* n_out) {
   if (n_out == nullptr || (capacity != 0 && out == nullptr)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_scan_timings: bad arguments");
   }
   ScanTimingLog& log = scanTimingLog();
   *n_out = static_cast<uint32_t>(log.used);
   for (size_t k = 0; k < log.used && k < capacity; ++k) {
      ScanLaunchTiming& launch = log.launches[k];
      HIP_TRY(hipEventSynchronize(launch.stop));
      HIP_TRY(hipEventElapsedTime(&launch.entry.ms, launch.start, launch.stop));
      out[k] = launch.entry;
   }
   return SILO_GPU_OK;
}

int silo_gpu_mutations_scan_batch(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint64_t* const* filters_dev, uint32_t n_filters, uint32_t pos_begin,
   uint32_t pos_end, uint32_t* const* counts_out_dev, void* stream
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || filters_dev == nullptr || counts_out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_scan_batch: bad arguments");
   }
   const silo_gpu_scan_range range{seqstore_id, pos_begin, pos_end};
   return silo_gpu_mutations_scan_ranges(store, &range, 1, filters_dev, n_filters, counts_out_dev, stream);
}

uint32_t silo_gpu_store_scan_planes(const silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size()) {
      return 0;
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   uint64_t positions_with[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // by number of plane rows
   for (const SeqStoreHost::Run& run : seqstore.layout.runs) {
      for (uint32_t p = run.begin; run.one_hot && p < run.end; ++p) {
         positions_with[(seqstore.layout.row_of[p + 1] - seqstore.layout.row_of[p]) & 7u] += 1;
      }
      positions_with[run.bits & 7u] += run.one_hot ? 0 : run.end - run.begin;
   }
   uint32_t most_common = seqstore.dev.n_bits;
   uint64_t most = 0;
   for (uint32_t bits = 0; bits < 8; ++bits) {  // (0: positions whose only frequent symbol is derived)
      if (positions_with[bits] > most) {
         most = positions_with[bits];
         most_common = bits;
      }
   }
   return most_common;
}

uint64_t silo_gpu_store_scan_rows(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t pos_begin, uint32_t pos_end) {
   if (store == nullptr || seqstore_id >= store->seqstores.size()) {
      return 0;
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   pos_end = std::min(pos_end, seqstore.dev.positions);
   if (pos_begin >= pos_end) {
      return 0;
   }
   if (seqstore.layout.row_of.empty()) {
      return static_cast<uint64_t>(pos_end - pos_begin) * seqstore.dev.n_bits;
   }
   return seqstore.layout.row_of[pos_end] - seqstore.layout.row_of[pos_begin];
}

uint64_t silo_gpu_store_scan_runs(const silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || !store->seqstores[seqstore_id].layout.has_implicit) {
      return 0;
   }
   return store->seqstores[seqstore_id].dev.n_missing_runs;
}

uint64_t silo_gpu_store_scan_sparse_keys(const silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || !store->seqstores[seqstore_id].layout.has_implicit) {
      return 0;
   }
   return store->seqstores[seqstore_id].sparse_sorted.size();
}

int silo_gpu_store_scan_prunable_granules(
   const silo_gpu_store* store, uint32_t seqstore_id, uint32_t cardinality, double min_proportion, uint64_t* out_skippable, uint64_t* out_total
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_skippable == nullptr || out_total == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_scan_prunable_granules: bad arguments");
   }
   const SeqStoreHost::Layout& layout = store->seqstores[seqstore_id].layout;
   *out_total = layout.escapes_sliced.packed_keys / ESCAPE_GRANULE_KEYS;
   *out_skippable = 0;
   for (size_t g = 0; g < layout.granule_heaviest.size(); ++g) {  // (empty where the store has no bounds)
      *out_skippable += granulePrunable(cardinality, layout.granule_without[g], layout.granule_heaviest[g], min_proportion) ? 1 : 0;
   }
   return SILO_GPU_OK;
}

int silo_gpu_store_scan_prunable_rows(
   const silo_gpu_store* store, uint32_t seqstore_id, uint32_t cardinality, double min_proportion, uint64_t* out_skippable, uint64_t* out_total
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || out_skippable == nullptr || out_total == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_scan_prunable_rows: bad arguments");
   }
   const SeqStoreHost::Layout& layout = store->seqstores[seqstore_id].layout;
   *out_total = 0;
   *out_skippable = 0;
   for (const SeqStoreHost::Run& run : layout.runs) {
      for (uint32_t row = run.one_hot ? layout.row_of[run.begin] : 0; run.one_hot && row < layout.row_of[run.end]; ++row) {
         *out_total += 1;
         if (row < layout.row_heaviest.size()) {  // (empty where the store has no bounds)
            *out_skippable += granulePrunable(cardinality, layout.row_without[row], layout.row_heaviest[row], min_proportion) ? 1 : 0;
         }
      }
   }
   return SILO_GPU_OK;
}

uint64_t silo_gpu_store_scan_covered_rows(const silo_gpu_store* store, uint32_t seqstore_id) {
   return store == nullptr || seqstore_id >= store->seqstores.size() ? 0 : store->seqstores[seqstore_id].layout.covered_rows;
}

uint64_t silo_gpu_store_scan_end_events(const silo_gpu_store* store, uint32_t seqstore_id) {
   return store == nullptr || seqstore_id >= store->seqstores.size() ? 0 : store->seqstores[seqstore_id].layout.end_events;
}

uint64_t silo_gpu_store_scan_residual_keys(const silo_gpu_store* store, uint32_t seqstore_id) {
   return store == nullptr || seqstore_id >= store->seqstores.size() ? 0 : store->seqstores[seqstore_id].layout.residual_keys;
}

uint64_t silo_gpu_store_scan_escapes(const silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || store->seqstores[seqstore_id].layout.escape_first.empty()) {
      return 0;
   }
   return store->seqstores[seqstore_id].layout.escape_first.back();
}

uint64_t silo_gpu_store_scan_overflow_keys(const silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || !store->seqstores[seqstore_id].layout.built) {
      return 0;
   }
   return store->seqstores[seqstore_id].layout.escapes_sliced.n_overflow;  // (0 in a store without slice-major keys)
}


int silo_gpu_mutations_scan(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint64_t* filter_dev, uint32_t pos_begin, uint32_t pos_end,
   uint32_t* counts_out_dev, void* stream
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || counts_out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_scan: bad arguments");
   }
   HIP_TRY(hipSetDevice(store->device));
   const SeqStoreDev& dev = store->seqstores[seqstore_id].dev;
   if (pos_begin > pos_end || pos_end > dev.positions) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "position range out of bounds");
   }
   if (pos_begin == pos_end || dev.n_scan == 0) {
      return SILO_GPU_OK;
   }
   auto hip_stream_early = static_cast<hipStream_t>(stream);
   if (filter_dev == nullptr) {
      // Full filter: add the cached totals of the unfiltered store instead of streaming the planes again.
      auto* mutable_store = const_cast<silo_gpu_store*>(store);  // the cache is logically const
      SeqStoreHost& seqstore = mutable_store->seqstores[seqstore_id];
      const size_t n_totals = static_cast<size_t>(dev.positions) * dev.n_scan;
      {
         const std::lock_guard<std::mutex> lock(mutable_store->mutex);
         if (!seqstore.totals_ready) {
            if (seqstore.d_totals.get() == nullptr) {
               HIP_TRY(seqstore.d_totals.alloc(n_totals));
            }
            HIP_TRY(hipMemsetAsync(seqstore.d_totals.get(), 0, n_totals * sizeof(uint32_t), hip_stream_early));
            const int rc = silo_gpu_mutations_scan(store, seqstore_id, store->d_ones.get(), 0, dev.positions, seqstore.d_totals.get(), stream);
            if (rc != SILO_GPU_OK) {
               return rc;
            }
            HIP_TRY(hipStreamSynchronize(hip_stream_early));  // other streams may read it from now on
            seqstore.totals_ready = true;
         }
      }
      const uint32_t n = (pos_end - pos_begin) * dev.n_scan;
      k_add_u32<<<(n + 255) / 256, 256, 0, hip_stream_early>>>(
         counts_out_dev, seqstore.d_totals.get() + static_cast<size_t>(pos_begin) * dev.n_scan, n
      );
      HIP_TRY(hipGetLastError());
      g_last_scan_kernel = "k_add_u32 (cached totals)";
      return SILO_GPU_OK;
   }
   const silo_gpu_scan_range range{seqstore_id, pos_begin, pos_end};
   return silo_gpu_mutations_scan_ranges(store, &range, 1, &filter_dev, 1, &counts_out_dev, stream);
}



}  // extern "C"
