// fused_select_rule.h — the host-side rule of silo_gpu_mutations_scan_select (silo_gpu_scan.hip): may the finish
// kernel of a scan overwrite a filter's count table and select its rows, and how many of its blocks take a ticket for the filter.
// Plain C++ without HIP, so that a stand-alone program can exercise it (tests/host_tools/fused_select_rule_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace silo_gpu_detail {

/// The part of a filter's count table that one range of a scan writes: positions [offset, offset + n_positions) of the table.
struct TableSpan {
   uint32_t offset;
   uint32_t n_positions;
};

/// Do the spans cover [0, total_positions) exactly — every position once, none beyond?  Only then is the scan the one writer of
/// every cell of the table and the table need not be cleared.  Empty spans are ignored; the order does not matter.
inline bool spansTileTable(std::vector<TableSpan> spans, uint32_t total_positions) {
   spans.erase(std::remove_if(spans.begin(), spans.end(), [](const TableSpan& span) { return span.n_positions == 0; }), spans.end());
   std::sort(spans.begin(), spans.end(), [](const TableSpan& a, const TableSpan& b) { return a.offset < b.offset; });
   uint64_t next = 0;
   for (const TableSpan& span : spans) {
      if (span.offset != next) {
         return false;  // a gap or an overlap
      }
      next += span.n_positions;
   }
   return next == total_positions;
}

/// Blocks of `positions_per_block` positions that the finish launches of a scan over ranges of these lengths have per filter, all
/// launches together (a launch takes up to DERIVED_MAX_RANGES ranges, each range whole blocks of its own): the tickets a filter's
/// row slot is to see before its header word is published.
inline uint32_t finishBlocks(const uint32_t* n_positions, size_t n_ranges, uint32_t positions_per_block) {
   uint64_t blocks = 0;
   for (size_t r = 0; r < n_ranges; ++r) {
      blocks += (static_cast<uint64_t>(n_positions[r]) + positions_per_block - 1) / positions_per_block;
   }
   return static_cast<uint32_t>(blocks);
}

}  // namespace silo_gpu_detail
