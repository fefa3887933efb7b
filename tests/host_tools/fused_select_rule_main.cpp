// fused_select_rule_main.cpp — a stand-alone program over the host-side rule of silo_gpu_mutations_scan_select
// (lapis-silo_amd/csrc/fused_select_rule.h): do the ranges of a call tile a filter's count table, and how many blocks of the
// finish launches take a ticket for a filter.  Built with -fsanitize=address,undefined and run by tests/test_fused_select_rule.py.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fused_select_rule.h"

using silo_gpu_detail::finishBlocks;
using silo_gpu_detail::spansTileTable;
using silo_gpu_detail::TableSpan;

namespace {

int failures = 0;

void expect(bool condition, const char* what) {
   if (!condition) {
      fprintf(stderr, "FAILED: %s\n", what);
      ++failures;
   }
}

/// `n_ranges` ranges of `length` positions back to back; the finish launches take 16 ranges each.
void backToBack(uint32_t n_ranges, uint32_t length, uint32_t blocks_per_range) {
   std::vector<TableSpan> spans;
   std::vector<uint32_t> lengths;
   for (uint32_t r = 0; r < n_ranges; ++r) {
      spans.push_back({r * length, length});
      lengths.push_back(length);
   }
   expect(spansTileTable(spans, n_ranges * length), "ranges back to back tile their table");
   expect(!spansTileTable(spans, n_ranges * length + 1), "a table one position longer is not tiled");
   expect(!spansTileTable(spans, n_ranges * length - 1), "a table one position shorter is not tiled");
   // the total does not depend on how the ranges are dealt to launches: summed per launch of 16 it is the same
   uint32_t per_launch = 0;
   for (size_t first = 0; first < lengths.size(); first += 16) {
      per_launch += finishBlocks(lengths.data() + first, std::min<size_t>(16, lengths.size() - first), 1024);
   }
   expect(finishBlocks(lengths.data(), lengths.size(), 1024) == n_ranges * blocks_per_range, "blocks of all finish launches");
   expect(per_launch == n_ranges * blocks_per_range, "blocks summed launch by launch");
}

}  // namespace

int main() {
   backToBack(1, 29903, 30);
   backToBack(16, 1273, 2);
   backToBack(17, 1024, 1);
   backToBack(17, 1025, 2);
   backToBack(12, 600, 1);

   expect(spansTileTable({{600, 97}, {0, 600}, {697, 3}}, 700), "the order of the ranges does not matter");
   expect(spansTileTable({{0, 600}, {600, 0}, {600, 100}, {5, 0}}, 700), "empty ranges are ignored");
   expect(!spansTileTable({{0, 600}, {601, 99}}, 700), "a gap of one position");
   expect(!spansTileTable({{10, 290}}, 2100), "positions 10 to 300 of 2100");
   expect(!spansTileTable({{0, 600}, {599, 101}}, 700), "an overlap of one position");
   expect(!spansTileTable({{0, 600}, {0, 600}}, 1200), "the same range twice");
   expect(!spansTileTable({{0, 600}, {600, 200}}, 700), "a range beyond the table");
   expect(!spansTileTable({}, 700), "no range at all");
   expect(!spansTileTable({{0, 0xFFFFFFFFu}, {0xFFFFFFFFu, 2}}, 1), "a sum past 2^32 does not wrap round to the table's length");
   expect(spansTileTable({{0, 0x80000000u}, {0x80000000u, 0x7FFFFFFFu}}, 0xFFFFFFFFu), "a table of 2^32 - 1 positions");

   const uint32_t odd[] = {1, 1023, 1024, 1025, 0, 2100, 0xFFFFFFFFu};
   expect(finishBlocks(odd, 7, 1024) == 1 + 1 + 1 + 2 + 0 + 3 + 4194304u, "partial blocks, an empty range, a range of 2^32 - 1 positions");
   expect(finishBlocks(odd, 0, 1024) == 0, "no range, no block");

   if (failures == 0) {
      printf("fused select rule ok\n");
   }
   return failures == 0 ? 0 : 1;
}
