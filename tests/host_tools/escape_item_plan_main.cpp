// escape_item_plan_main.cpp — a stand-alone program over the host-side plan of a launch of k_scan_escapes_sliced
// (lapis-silo_amd/csrc/escape_item_plan.h): the items of a launch, their order and the blocks that walk them.  Built with
// -fsanitize=address,undefined and run by tests/test_escape_item_plan.py.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "escape_item_plan.h"

using namespace silo_gpu_detail;

namespace {

int failures = 0;

void expect(bool condition, const char* what, uint32_t a = 0, uint32_t b = 0, int c = 0) {
   if (!condition) {
      fprintf(stderr, "FAILED: %s (%u entries, %u slices, knob %d)\n", what, a, b, c);
      ++failures;
   }
}

/// Walks the items as the kernel's blocks do — block b: b, b + G, ... below n_items, in 32-bit arithmetic — and checks the plan.
void check(const std::vector<EscapeEntryShape>& entries, uint32_t n_slices, uint32_t passes, uint32_t places, int knob) {
   const uint32_t n = static_cast<uint32_t>(entries.size());
   const EscapeItemPlan plan = planEscapeItems(entries.data(), n, n_slices, passes, places, knob);
   expect(plan.ok, "the plan is made", n, n_slices, knob);
   if (!plan.ok) {
      return;
   }
   expect(plan.block_keys % ESCAPE_PLAN_GRANULE_KEYS == 0 && plan.block_keys >= ESCAPE_PLAN_GRANULE_KEYS &&
             plan.block_keys <= ESCAPE_PLAN_GRANULES_PER_ITEM * ESCAPE_PLAN_GRANULE_KEYS,
          "an item is 1 to 64 whole granules", n, n_slices, knob);
   // the entries: a permutation — the caller's order, or the never-pruned ones first and each group in the caller's order —; every
   // key of a slice lies in a share
   std::vector<uint32_t> seen(n, 0);
   uint64_t items = 0;
   for (uint32_t k = 0; k < n; ++k) {
      expect(plan.order[k] < n, "an entry of the caller's", n, n_slices, knob);
      if (plan.order[k] >= n) {
         return;
      }
      ++seen[plan.order[k]];
      const EscapeEntryShape& entry = entries[plan.order[k]];
      if (k > 0) {
         const EscapeEntryShape& before = entries[plan.order[k - 1]];
         if (plan.never_pruned_first) {
            expect(before.prunable <= entry.prunable, "never-pruned entries come first", n, n_slices, knob);
            expect(before.prunable != entry.prunable || plan.order[k - 1] < plan.order[k], "a group keeps the caller's order", n, n_slices, knob);
         } else {
            expect(plan.order[k - 1] < plan.order[k], "the caller's order", n, n_slices, knob);
         }
      }
      expect(plan.items_per_slice[k] >= 1, "an item per slice at least", n, n_slices, knob);
      expect(static_cast<uint64_t>(plan.items_per_slice[k]) * plan.block_keys >= entry.most_keys, "the shares of a slice hold its keys", n, n_slices, knob);
      expect(static_cast<uint64_t>(plan.items_per_slice[k] - 1u) * plan.block_keys < std::max<uint32_t>(1, entry.most_keys), "no share beyond the keys", n, n_slices, knob);
      expect(plan.first_item[k] == items, "an entry's items follow those of the entries before", n, n_slices, knob);
      items += static_cast<uint64_t>(plan.items_per_slice[k]) * n_slices;
   }
   for (uint32_t k = 0; k < n; ++k) {
      expect(seen[k] == 1, "every entry once", n, n_slices, knob);
   }
   expect(items == plan.n_items && items <= ESCAPE_PLAN_MAX_ITEMS, "the items are counted without wrapping", n, n_slices, knob);
   // the grid
   const uint32_t resident = std::max<uint32_t>(1, places / passes);
   const uint32_t want_grid = knob == 0 ? plan.n_items : std::min(plan.n_items, knob > 0 ? static_cast<uint32_t>(knob) : resident);
   expect(plan.grid == want_grid && plan.grid >= 1, "the grid", n, n_slices, knob);
   if (knob < 0) {
      expect(static_cast<uint64_t>(plan.grid) * passes <= std::max(places, passes), "grid.x * grid.z stays within the places", n, n_slices, knob);
   }
   expect(static_cast<uint64_t>(plan.n_items) + plan.grid <= 0xFFFFFFFFull, "item + G does not wrap", n, n_slices, knob);
   if (plan.n_items > (1u << 22)) {
      return;  // (the walk below is for the sizes a test can afford)
   }
   // the deal: every item exactly once; an item decodes to a (entry, slice, share) of its own
   std::vector<uint8_t> dealt(plan.n_items, 0);
   bool prunable_seen = false;
   for (uint32_t item = 0; item < plan.n_items; ++item) {
      const EscapeItem at = escapeItemOf(plan, n, item);
      expect(at.entry < n && at.slice < n_slices && at.share < plan.items_per_slice[at.entry], "an item lies inside its entry", n, n_slices, knob);
      if (at.entry >= n) {
         return;
      }
      expect(plan.first_item[at.entry] + at.slice * plan.items_per_slice[at.entry] + at.share == item, "(entry, slice, share) numbers the item", n, n_slices, knob);
      const bool prunable = entries[plan.order[at.entry]].prunable;
      expect(!plan.never_pruned_first || prunable || !prunable_seen, "never-pruned items are numbered first", n, n_slices, knob);
      prunable_seen = prunable_seen || prunable;
   }
   for (uint32_t block = 0; block < plan.grid; ++block) {
      for (uint32_t item = block; item < plan.n_items; item += plan.grid) {
         ++dealt[item];
      }
   }
   bool once = true;
   for (uint32_t item = 0; item < plan.n_items; ++item) {
      once = once && dealt[item] == 1;
   }
   expect(once, "every item is dealt exactly once", n, n_slices, knob);
}

/// The entries of a launch: kinds in turn (escape keys that may be pruned, gap events, end events, residual keys), `scale` keys
/// to the largest slice of the first, one entry without keys.
std::vector<EscapeEntryShape> launchOf(uint32_t n_entries, uint32_t n_slices, uint32_t scale, bool pruning) {
   std::vector<EscapeEntryShape> entries;
   for (uint32_t k = 0; k < n_entries; ++k) {
      const uint32_t keys_per_slice = k % 5 == 4 ? 0 : scale / (1u + k % 4 * 7u) + k;
      EscapeEntryShape entry{};
      entry.most_keys = keys_per_slice + ESCAPE_PLAN_GRANULE_KEYS - 1u;
      entry.keys = static_cast<uint64_t>(keys_per_slice) * n_slices * 3u / 4u;
      entry.prunable = pruning && k % 4 == 1;
      entries.push_back(entry);
   }
   return entries;
}

}  // namespace

int main() {
   for (uint32_t n_entries = 1; n_entries <= ESCAPE_PLAN_MAX_ENTRIES; ++n_entries) {
      for (const uint32_t n_slices : {1u, 2u, 512u}) {
         for (const uint32_t scale : {1u, 5000u, 300000u}) {
            for (const bool pruning : {false, true}) {
               const std::vector<EscapeEntryShape> entries = launchOf(n_entries, n_slices, scale, pruning);
               for (const uint32_t passes : {1u, 2u}) {
                  const uint32_t n_items = planEscapeItems(entries.data(), n_entries, n_slices, passes, 512, 0).n_items;
                  for (const int knob : {-1, 0, 1, 2, 3, 5, static_cast<int>(n_items) - 1, static_cast<int>(n_items), static_cast<int>(n_items) + 1, 1 << 30}) {
                     check(entries, n_slices, passes, 512, knob);  // (n_items - 1 = 0 where there is one item: the default)
                  }
                  // the blocks the chip holds: unknown, one, fewer than passes, 256 (one block per CU), 512
                  for (const uint32_t places : {0u, 1u, 256u, 512u, 0xFFFFFFFFu}) {
                     check(entries, n_slices, passes, places, -1);
                  }
               }
            }
         }
      }
   }
   {  // every G from 1 to beyond the items of a small launch
      const std::vector<EscapeEntryShape> entries = launchOf(4, 2, 40000, true);
      for (int knob = 1; knob <= 64; ++knob) {
         check(entries, 2, 1, 512, knob);
      }
   }
   {  // the headline's shape: 77 slices; end events, residual keys, prunable escape keys, gap events — 7 301 never-pruned granules
      // over 512 places make items of 14, numbered first
      std::vector<EscapeEntryShape> entries = {
         {258442 + 4095, 19900000, false}, {26 + 4095, 1976, false}, {957394 + 4095, 73719808, true}, {129871 + 4095, 10000000, false}};
      for (const int knob : {0, -1, 512}) {
         check(entries, 77, 1, 512, knob);
         const EscapeItemPlan plan = planEscapeItems(entries.data(), 4, 77, 1, 512, knob);
         expect(plan.ok && plan.never_pruned_first && plan.block_keys == 14u * ESCAPE_PLAN_GRANULE_KEYS, "items of 14 granules");
         expect(plan.order[0] == 0 && plan.order[1] == 1 && plan.order[2] == 3 && plan.order[3] == 2, "ends, residual, gaps, then the prunable keys");
         expect(plan.grid == (knob == 0 ? plan.n_items : 512u), "one block per item, or 512 blocks");
      }
      expect(planEscapeItems(entries.data(), 4, 77, 2, 512, 0).block_keys == 28u * ESCAPE_PLAN_GRANULE_KEYS, "two passes share the places");
      expect(planEscapeItems(entries.data(), 4, 77, 1, 512, 1).block_keys == 64u * ESCAPE_PLAN_GRANULE_KEYS, "planned as for one place: the longest items");
      {  // a tenth of the rows: the never-pruned items would be a single granule — the caller's order, granules / 1280
         const std::vector<EscapeEntryShape> small = {
            {250000 + 4095, 1990000, false}, {26 + 4095, 200, false}, {921000 + 4095, 7371980, true}, {125000 + 4095, 1000000, false}};
         check(small, 8, 1, 512, 0);
         const EscapeItemPlan plan = planEscapeItems(small.data(), 4, 8, 1, 512, 0);
         expect(plan.ok && !plan.never_pruned_first && plan.block_keys == 1u * ESCAPE_PLAN_GRANULE_KEYS, "2 530 granules / 1280 = 1");
         expect(plan.order[0] == 0 && plan.order[1] == 1 && plan.order[2] == 2 && plan.order[3] == 3, "the caller's order");
      }
      {  // twelve genes' worth of prunable keys beside few gap events: the caller's order, granules / 1280
         const std::vector<EscapeEntryShape> genes = {{400000 + 4095, 30000000, true}, {2000 + 4095, 150000, false}, {300000 + 4095, 22000000, true}, {1500 + 4095, 100000, false}};
         check(genes, 77, 1, 512, 0);
         const EscapeItemPlan plan = planEscapeItems(genes.data(), 4, 77, 1, 512, 0);
         expect(plan.ok && !plan.never_pruned_first && plan.block_keys == 9u * ESCAPE_PLAN_GRANULE_KEYS, "12 757 granules / 1280 = 9");
      }
      entries[2].prunable = false;  // the exact scan of the same store
      const EscapeItemPlan exact = planEscapeItems(entries.data(), 4, 77, 1, 512, 0);
      expect(exact.ok && !exact.never_pruned_first && exact.block_keys == 19u * ESCAPE_PLAN_GRANULE_KEYS && exact.grid == exact.n_items, "nothing prunable: granules / 1280");
      expect(exact.order[0] == 0 && exact.order[1] == 1 && exact.order[2] == 2 && exact.order[3] == 3, "nothing prunable: the caller's order");
   }
   {  // sums past 2^32: the largest slices there can be, in every entry
      std::vector<EscapeEntryShape> entries(ESCAPE_PLAN_MAX_ENTRIES, EscapeEntryShape{0xFFFFFFFFu, 0xFFFFFFFFull * 512u, false});
      check(entries, 512, 1, 512, -1);   // 64 granules to an item: 2^27 items
      check(entries, 512, 8, 512, 0);
      for (EscapeEntryShape& entry : entries) {
         entry.keys = 1;  // (a launch that claims few keys: one granule to an item would give 2^33 items)
      }
      const EscapeItemPlan plan = planEscapeItems(entries.data(), ESCAPE_PLAN_MAX_ENTRIES, 512, 1, 512, 0);
      expect(!plan.ok, "more items than the kernel numbers: refused, not wrapped");
      for (EscapeEntryShape& entry : entries) {
         entry.keys = 0xFFFFFFFFull * 512u;
      }
      entries[3].prunable = true;
      check(entries, 512, 1, 512, -1);
   }
   {  // bad arguments
      const EscapeEntryShape one{5000, 900, false};
      expect(!planEscapeItems(nullptr, 1, 1, 1, 512, 0).ok, "no entries");
      expect(!planEscapeItems(&one, 0, 1, 1, 512, 0).ok, "zero entries");
      expect(!planEscapeItems(&one, ESCAPE_PLAN_MAX_ENTRIES + 1, 1, 1, 512, 0).ok, "too many entries");
      expect(!planEscapeItems(&one, 1, 0, 1, 512, 0).ok, "zero slices");
      expect(!planEscapeItems(&one, 1, 1, 0, 512, 0).ok, "zero passes");
   }
   if (failures == 0) {
      printf("escape item plan ok\n");
   }
   return failures == 0 ? 0 : 1;
}
