// escape_item_plan.h — the host-side plan of a launch of k_scan_escapes_sliced (silo_gpu_scan_keys.hip; DESIGN.md §3, "The escape
// pass"): how the keys of the launch's entries are cut into items, in which order the items are numbered, and how many blocks walk
// them.  An item is a (entry, slice, share) triple: at most block_keys keys of one slice of one entry, whole granules.  Block b of
// a grid of G blocks takes the items b, b + G, b + 2 G, ... below n_items.
// Plain C++ without HIP, so that a stand-alone program can exercise it (tests/host_tools/escape_item_plan_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace silo_gpu_detail {

constexpr uint32_t ESCAPE_PLAN_MAX_ENTRIES = 16;         // = ESCAPE_MAX_RANGES (store_internal.h)
constexpr uint32_t ESCAPE_PLAN_GRANULE_KEYS = 4096;      // = ESCAPE_GRANULE_KEYS
constexpr uint32_t ESCAPE_PLAN_GRANULES_PER_ITEM = 64;   // = ESCAPE_GRANULES_PER_BLOCK: an item's granules are listed one per lane of a wave
constexpr uint32_t ESCAPE_PLAN_MAX_ITEMS = 1u << 30;     // item + G must not wrap in the kernel's loop

/// One entry of a launch: the keys of one stream (escape keys, gap events, end events, residual keys) of one range.
struct EscapeEntryShape {
   uint32_t most_keys;  // of one slice, from the granule its first key lies in: keys + ESCAPE_PLAN_GRANULE_KEYS - 1 (0 = no slice has keys)
   uint64_t keys;       // of all slices
   bool prunable;       // the launch may skip granules of this entry (it has bounds per granule)
};

struct EscapeItemPlan {
   bool ok;              // false: more than ESCAPE_PLAN_MAX_ITEMS items, or bad arguments; nothing else is valid then
   uint32_t block_keys;  // keys of an item at most: whole granules
   uint32_t n_items;
   uint32_t grid;        // blocks (grid.x); grid.z = passes stays the caller's
   bool never_pruned_first;
   // the entries in the order of their items — the caller's, or the never-pruned ones first and each group in the caller's order
   uint32_t order[ESCAPE_PLAN_MAX_ENTRIES];            // [k] = the caller's index of the k-th entry
   uint32_t first_item[ESCAPE_PLAN_MAX_ENTRIES];       // [k] = the items of the entries before the k-th
   uint32_t items_per_slice[ESCAPE_PLAN_MAX_ENTRIES];  // [k] >= 1: the k-th entry's items are numbered slice by slice
};

/// The (entry in the plan's order, slice, share) of an item: the arithmetic k_scan_escapes_sliced does on the device.
struct EscapeItem {
   uint32_t entry;
   uint32_t slice;
   uint32_t share;
};
inline EscapeItem escapeItemOf(const EscapeItemPlan& plan, uint32_t n_entries, uint32_t item) {
   uint32_t k = 0;
   while (k + 1u < n_entries && item >= plan.first_item[k + 1u]) {
      ++k;
   }
   const uint32_t within = item - plan.first_item[k];
   return EscapeItem{k, within / plan.items_per_slice[k], within % plan.items_per_slice[k]};
}

/// Items of one slice of an entry — as many as its slice with the most keys needs, one at least — for items of `block_keys` keys.
inline uint64_t escapeItemsPerSlice(const EscapeEntryShape& entry, uint32_t block_keys) {
   return std::max<uint64_t>(1, (static_cast<uint64_t>(entry.most_keys) + block_keys - 1) / block_keys);
}

/// `places` = blocks of the instantiation the chip holds at once (0 = unknown: as one); `passes` = grid.z; `knob` =
/// SILO_GPU_TUNE_ESCAPE_BLOCKS: 0 one block per item, < 0 resident blocks (places / passes), n > 0 exactly min(n, n_items) blocks —
/// and then the plan is made as for a chip of n places, so that a test reaches every kind of plan with a small store.
///
/// Order and item size.  A launch that may prune reads nearly all its keys from the entries it never prunes
/// (profiles/r05_pruned_keys.md).  Where those give every place two granules or more, their items are numbered FIRST and are the
/// never-pruned granules / places long (no shorter than the prunable granules / 1280): the chip fills with the long items and the
/// short prunable ones fill the places as they fall free (profiles/r10_escape_items.md: 69 -> 57 us on the headline).  Otherwise —
/// nothing prunable, or never-pruned items of a single granule, which live no longer than an item that finds nothing to do —
/// the entries keep the caller's order and an item is the launch's granules / 1280 long, about five shares to a place
/// (profiles/r03_notes.md): with one-granule items first, the 1 M sequence store lost 10 us (same file).
inline EscapeItemPlan planEscapeItems(const EscapeEntryShape* entries, uint32_t n_entries, uint32_t n_slices, uint32_t passes, uint32_t places, int knob) {
   EscapeItemPlan plan{};
   if (entries == nullptr || n_entries == 0 || n_entries > ESCAPE_PLAN_MAX_ENTRIES || n_slices == 0 || passes == 0) {
      return plan;
   }
   const uint32_t resident = knob > 0 ? static_cast<uint32_t>(knob) : std::max<uint32_t>(1, places / passes);  // grid.x * grid.z stays within one round of the places
   bool prunable = false;
   uint64_t keys = 0, never_pruned_keys = 0;
   for (uint32_t k = 0; k < n_entries; ++k) {
      prunable = prunable || entries[k].prunable;
      keys += entries[k].keys;
      never_pruned_keys += entries[k].prunable ? 0 : entries[k].keys;
   }
   const auto granulesOf = [](uint64_t n) { return (n + ESCAPE_PLAN_GRANULE_KEYS - 1) / ESCAPE_PLAN_GRANULE_KEYS; };
   const uint64_t never_pruned_per_place = granulesOf(never_pruned_keys) / resident;
   const bool never_pruned_first = prunable && never_pruned_per_place >= 2;
   const uint64_t granules = never_pruned_first ? std::max(never_pruned_per_place, granulesOf(keys - never_pruned_keys) * passes / 1280)
                                                : granulesOf(keys) * passes / 1280;
   const uint32_t block_granules = static_cast<uint32_t>(std::min<uint64_t>(ESCAPE_PLAN_GRANULES_PER_ITEM, std::max<uint64_t>(1, granules)));
   plan.block_keys = block_granules * ESCAPE_PLAN_GRANULE_KEYS;
   uint64_t items = 0;
   for (uint32_t k = 0; k < n_entries; ++k) {
      items += escapeItemsPerSlice(entries[k], plan.block_keys) * n_slices;
   }
   if (items > ESCAPE_PLAN_MAX_ITEMS) {
      return plan;
   }
   uint32_t n = 0, first = 0;
   for (const bool pruned : {false, true}) {  // (one sweep in the caller's order where nothing is put first)
      for (uint32_t k = 0; k < n_entries; ++k) {
         if (never_pruned_first ? entries[k].prunable != pruned : pruned) {
            continue;
         }
         plan.order[n] = k;
         plan.first_item[n] = first;
         plan.items_per_slice[n] = static_cast<uint32_t>(escapeItemsPerSlice(entries[k], plan.block_keys));
         first += plan.items_per_slice[n] * n_slices;  // (<= items <= ESCAPE_PLAN_MAX_ITEMS)
         ++n;
      }
   }
   plan.n_items = first;
   plan.grid = knob == 0 ? plan.n_items : std::min(plan.n_items, resident);
   plan.never_pruned_first = never_pruned_first;
   plan.ok = true;
   return plan;
}

}  // namespace silo_gpu_detail
