// silo_gpu_grouped.hip — the grouped count behind MutationsOverTime: for a few listed (position, symbol) pairs, the rows of a
// filter that carry the symbol and the rows that have any valid symbol there, counted per group of rows (a date range) instead
// of once per filter.  Five launches on the caller's stream:
//   k_assign_groups             a uint16 group id per row (filter x date ranges), |filter ∩ range| per group
//   k_grouped_position_counts   per listed mutation and group: H_sym (rows with the symbol) and H_stored (rows with any coded
//                               symbol) from the code planes / one-hot rows; for derived positions also the rows whose symbol
//                               sits in an extra plane (no valid symbol)
//   k_grouped_escapes           the position's escape keys into H_sym / H_stored
//   k_grouped_missing_runs, k_grouped_sparse_keys   rows without a valid symbol at the listed derived positions: runs of the
//                               missing symbol (one pass over all runs for all positions), sparse ambiguity keys
//   k_finish_grouped            count / coverage per (mutation, group), added to the caller's table
// And the grouped count behind QueriesOverTime (K8, silo_gpu_filters_grouped): many filter bitsets against the same group ids.
//   k_assign_groups             as above, over the base filter
//   k_grouped_filter_counts     per filter and group: the rows of the filter in the group, added to the caller's table
#include <algorithm>
#include <cstring>
#include <numeric>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint16_t NO_GROUP = 0xFFFFu;
constexpr uint32_t GROUP_THREADS = 256;
constexpr uint32_t POSITION_THREADS = 256;   // one row word per thread: a block covers 256 words = 16 384 rows
constexpr uint32_t MUTATIONS_PER_BLOCK = 16;  // mutations a block of k_grouped_position_counts counts, the groups of its rows decoded once
constexpr uint32_t WORD_SEGMENTS = 4;          // distinct groups of a word kept as (group, mask) pairs; beyond: per row
constexpr uint32_t FILTERS_PER_BLOCK = 8;      // filters a block of k_grouped_filter_counts counts: an LDS histogram of 32 KiB at 1 024 groups
constexpr uint32_t MAX_EXTRA = 16;
constexpr uint32_t NO_POSITION = 0xFFFFFFFFu;

/// The per-mutation tables of a launch (device pointers into the caller's scratch).
struct GroupedArgs {
   SeqStoreDev dev;
   uint16_t* groups;              // [row_words * 64]
   const uint32_t* mut_position;  // [M]
   const uint32_t* mut_scan;      // [M] scan symbol index
   const uint32_t* mut_derived;   // [M] index among the listed derived positions (counts rows without a symbol), NO_POSITION otherwise
   const uint32_t* mut_first;     // [M] 1: the first mutation of its derived position (counts the extra planes)
   const uint32_t* derived_positions;  // [n_derived] ascending
   const uint32_t* sparse_range;  // [n_derived][2] the sparse keys of a derived position
   const uint32_t* bound_from;    // [G] the ranges sorted by their start
   const uint32_t* bound_to;
   const uint32_t* bound_group;   // the group (request index) of a sorted range
   uint32_t* cardinality;         // [G]
   uint32_t* h_sym;               // [M][G]
   uint32_t* h_stored;            // [M][G]
   uint32_t* without_symbol;      // [n_derived][G]
   const uint64_t* sparse_keys;
   uint32_t n_mutations;
   uint32_t n_groups;
   uint32_t n_derived;
   uint32_t sequence_count;
   uint32_t n_extra;
   uint8_t extra_symbols[MAX_EXTRA];  // symbols kept in extra planes (none of them a valid symbol)
};

/// grid = (row_words * 64 / GROUP_THREADS): a thread per row.  The sorted range bounds sit in LDS; a row's group is the range
/// whose start is the last one <= its date, if the date is also <= that range's end.  Padding rows and NULL dates get none.
__global__ __launch_bounds__(GROUP_THREADS) void k_assign_groups(const GroupedArgs args, const uint64_t* __restrict__ filter, const uint32_t* __restrict__ dates) {
   __shared__ uint32_t s_from[SILO_GPU_MAX_DATE_RANGES];
   __shared__ uint32_t s_to[SILO_GPU_MAX_DATE_RANGES];
   __shared__ uint32_t s_group[SILO_GPU_MAX_DATE_RANGES];
   __shared__ uint32_t s_count[SILO_GPU_MAX_DATE_RANGES];
   const uint32_t n = args.n_groups;
   for (uint32_t i = threadIdx.x; i < n; i += GROUP_THREADS) {
      s_from[i] = args.bound_from[i];
      s_to[i] = args.bound_to[i];
      s_group[i] = args.bound_group[i];
      s_count[i] = 0;
   }
   __syncthreads();
   const uint32_t row = blockIdx.x * GROUP_THREADS + threadIdx.x;  // < row_words * 64 (grid is exact)
   uint32_t group = NO_GROUP;
   // the valid mask: rows past sequence_count never count, whatever a filter's padding bits say
   const bool selected = row < args.sequence_count && (filter == nullptr || ((filter[row >> 6] >> (row & 63u)) & 1ull) != 0);
   if (selected) {
      const uint32_t date = dates[row];
      uint32_t lo = 0, hi = n;
      while (lo < hi) {
         const uint32_t mid = (lo + hi) >> 1;
         if (s_from[mid] <= date) {
            lo = mid + 1;
         } else {
            hi = mid;
         }
      }
      if (lo > 0 && date != 0 && date <= s_to[lo - 1]) {  // (every start is >= 1: NULL dates fall in no range)
         group = s_group[lo - 1];
         atomicAdd(&s_count[group], 1u);
      }
   }
   args.groups[row] = static_cast<uint16_t>(group);
   __syncthreads();
   for (uint32_t i = threadIdx.x; i < n; i += GROUP_THREADS) {
      if (s_count[i] != 0) {
         atomicAdd(&args.cardinality[i], s_count[i]);
      }
   }
}

/// The 64 group ids of row word `word` as up to WORD_SEGMENTS (group, row mask) pairs, in the order the groups first occur
/// (unused pairs: NO_GROUP, 0; rows without a group are in no mask).  true: the word has more groups than that — the masks are
/// incomplete and the word has to be taken row by row.  Without a word: no pair.
__device__ __forceinline__ bool decodeWordGroups(
   const uint16_t* groups, uint32_t word, bool has_word, uint32_t (&seg_group)[WORD_SEGMENTS], uint64_t (&seg_mask)[WORD_SEGMENTS]
) {
#pragma unroll
   for (uint32_t s = 0; s < WORD_SEGMENTS; ++s) {
      seg_group[s] = NO_GROUP;
      seg_mask[s] = 0;
   }
   bool row_by_row = false;
   if (has_word) {
      const uint4* ids = reinterpret_cast<const uint4*>(groups + static_cast<size_t>(word) * 64u);
#pragma unroll
      for (uint32_t chunk = 0; chunk < 8; ++chunk) {
         const uint4 v = ids[chunk];
         const uint32_t pairs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
         for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t g = (pairs[k >> 1] >> ((k & 1u) * 16u)) & 0xFFFFu;
            const uint64_t bit = 1ull << (chunk * 8u + k);
            if (g == NO_GROUP) {
               continue;
            }
            bool placed = false;
#pragma unroll
            for (uint32_t s = 0; s < WORD_SEGMENTS; ++s) {
               if (!placed && (seg_group[s] == g || seg_group[s] == NO_GROUP)) {
                  seg_group[s] = g;
                  seg_mask[s] |= bit;
                  placed = true;
               }
            }
            row_by_row |= !placed;
         }
      }
   }
   return row_by_row;
}

/// grid = (row_words / POSITION_THREADS rounded up, mutation batches of MUTATIONS_PER_BLOCK).  A thread owns one row word: it
/// reads the 64 group ids once and keeps up to WORD_SEGMENTS (group, row mask) pairs (rows are in (lineage, date) order: a word
/// rarely spans more groups); a word with more goes row by row.  Per mutation the word's symbol / stored / no-symbol masks are
/// split by those pairs into LDS histograms, which are flushed with one global add per non-zero entry.
__global__ __launch_bounds__(POSITION_THREADS) void k_grouped_position_counts(const GroupedArgs args) {
   __shared__ uint32_t s_hist[3 * SILO_GPU_MAX_DATE_RANGES];  // [group][sym, stored, no symbol]
   const uint32_t n_groups = args.n_groups;
   const uint32_t row_words = args.dev.row_words;
   const uint32_t word = blockIdx.x * POSITION_THREADS + threadIdx.x;
   const bool has_word = word < row_words;
   for (uint32_t i = threadIdx.x; i < 3u * n_groups; i += POSITION_THREADS) {
      s_hist[i] = 0;
   }
   uint32_t seg_group[WORD_SEGMENTS];
   uint64_t seg_mask[WORD_SEGMENTS];
   const bool row_by_row = decodeWordGroups(args.groups, word, has_word, seg_group, seg_mask);
   __syncthreads();
   const uint32_t m_end = min(args.n_mutations, (blockIdx.y + 1u) * MUTATIONS_PER_BLOCK);
   for (uint32_t m = blockIdx.y * MUTATIONS_PER_BLOCK; m < m_end; ++m) {
      const uint32_t position = args.mut_position[m];
      const PositionLayout layout = layoutOf(args.dev, position);
      const uint32_t code = codeOfSymbol(layout, args.mut_scan[m]);
      const bool count_extra = args.mut_first[m] != 0;  // (uniform)
      uint64_t sym = 0, stored = 0, none = 0;
      if (has_word) {
         for (uint32_t plane = 0; plane < layout.bits; ++plane) {
            stored |= layout.rows[static_cast<size_t>(plane) * row_words + word];  // code != 0 / a one-hot row
         }
         if (code != CODE_ESCAPED && code != CODE_IMPLICIT) {
            sym = decodeCodeWord(layout, row_words, code, word);
         }
         if (count_extra) {
            for (uint32_t e = 0; e < args.n_extra; ++e) {
               none |= planePtr(args.dev, position, args.extra_symbols[e])[word];
            }
         }
      }
      if (!row_by_row) {
#pragma unroll
         for (uint32_t s = 0; s < WORD_SEGMENTS; ++s) {
            if (seg_mask[s] != 0) {
               uint32_t* h = s_hist + seg_group[s] * 3u;
               const uint32_t c_sym = static_cast<uint32_t>(__popcll(sym & seg_mask[s]));
               const uint32_t c_stored = static_cast<uint32_t>(__popcll(stored & seg_mask[s]));
               const uint32_t c_none = static_cast<uint32_t>(__popcll(none & seg_mask[s]));
               if (c_sym != 0) {
                  atomicAdd(h, c_sym);
               }
               if (c_stored != 0) {
                  atomicAdd(h + 1, c_stored);
               }
               if (c_none != 0) {
                  atomicAdd(h + 2, c_none);
               }
            }
         }
      } else {
         for (uint64_t rest = sym | stored | none; rest != 0; rest &= rest - 1) {
            const uint32_t bit = static_cast<uint32_t>(__builtin_ctzll(rest));
            const uint32_t g = args.groups[static_cast<size_t>(word) * 64u + bit];
            if (g != NO_GROUP) {
               uint32_t* h = s_hist + g * 3u;
               if ((sym >> bit) & 1ull) {
                  atomicAdd(h, 1u);
               }
               if ((stored >> bit) & 1ull) {
                  atomicAdd(h + 1, 1u);
               }
               if ((none >> bit) & 1ull) {
                  atomicAdd(h + 2, 1u);
               }
            }
         }
      }
      __syncthreads();
      const size_t table = static_cast<size_t>(m) * n_groups;
      const uint32_t derived = args.mut_derived[m];
      for (uint32_t g = threadIdx.x; g < n_groups; g += POSITION_THREADS) {
         const uint32_t c_sym = s_hist[g * 3u], c_stored = s_hist[g * 3u + 1u], c_none = s_hist[g * 3u + 2u];
         if (c_sym != 0) {
            atomicAdd(&args.h_sym[table + g], c_sym);
         }
         if (c_stored != 0) {
            atomicAdd(&args.h_stored[table + g], c_stored);
         }
         if (c_none != 0 && derived != NO_POSITION) {
            atomicAdd(&args.without_symbol[static_cast<size_t>(derived) * n_groups + g], c_none);
         }
         s_hist[g * 3u] = 0;
         s_hist[g * 3u + 1u] = 0;
         s_hist[g * 3u + 2u] = 0;
      }
      __syncthreads();
   }
}

/// grid = (mutation, key blocks): the escape keys of the mutation's position (valid symbols without a code there).  Every key of
/// a selected row counts as stored; those of the requested symbol count as the symbol too.
__global__ __launch_bounds__(256) void k_grouped_escapes(const GroupedArgs args) {
   const uint32_t m = blockIdx.x;
   if (args.dev.escape_first == nullptr) {
      return;  // (uniform) no position of the store has keys
   }
   const uint32_t position = args.mut_position[m];
   const uint32_t scan_index = args.mut_scan[m];
   const uint32_t begin = args.dev.escape_first[position];
   const uint32_t end = args.dev.escape_first[position + 1];
   const size_t table = static_cast<size_t>(m) * args.n_groups;
   for (uint32_t i = begin + blockIdx.y * 256u + threadIdx.x; i < end; i += gridDim.y * 256u) {
      const uint64_t key = args.dev.escapes[i];
      const uint32_t sequence = static_cast<uint32_t>(key);
      const uint32_t g = args.groups[sequence];
      if (g != NO_GROUP) {
         atomicAdd(&args.h_stored[table + g], 1u);
         if (((key >> 32) & 31u) == scan_index) {
            atomicAdd(&args.h_sym[table + g], 1u);
         }
      }
   }
}

/// A thread per run of the missing symbol (grid-stride): a selected row's run adds one to every listed derived position it
/// covers — found by a binary search over those positions (in LDS) — so that the runs are read once for all mutations.
__global__ __launch_bounds__(256) void k_grouped_missing_runs(const GroupedArgs args) {
   __shared__ uint32_t s_positions[SILO_GPU_MAX_GROUPED_MUTATIONS];
   const uint32_t n = args.n_derived;
   for (uint32_t i = threadIdx.x; i < n; i += 256u) {
      s_positions[i] = args.derived_positions[i];
   }
   __syncthreads();
   for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < args.dev.n_missing_runs; i += gridDim.x * 256u) {
      const uint64_t key = args.dev.missing_run_keys[i];
      const uint32_t g = args.groups[static_cast<uint32_t>(key >> 32)];
      if (g == NO_GROUP) {
         continue;
      }
      const uint32_t start = static_cast<uint32_t>(key);
      const uint32_t end = args.dev.missing_run_ends[i];
      uint32_t lo = 0, hi = n;
      while (lo < hi) {
         const uint32_t mid = (lo + hi) >> 1;
         if (s_positions[mid] < start) {
            lo = mid + 1;
         } else {
            hi = mid;
         }
      }
      for (uint32_t k = lo; k < n && s_positions[k] < end; ++k) {
         atomicAdd(&args.without_symbol[static_cast<size_t>(k) * args.n_groups + g], 1u);
      }
   }
}

/// grid = (derived position, key blocks): the sparse keys (ambiguity codes, or the missing symbol where it has neither runs nor
/// a plane) of the position; a selected row's key is a row without a valid symbol.
__global__ __launch_bounds__(256) void k_grouped_sparse_keys(const GroupedArgs args) {
   const uint32_t k = blockIdx.x;
   const uint32_t begin = args.sparse_range[2u * k];
   const uint32_t end = args.sparse_range[2u * k + 1u];
   for (uint32_t i = begin + blockIdx.y * 256u + threadIdx.x; i < end; i += gridDim.y * 256u) {
      const uint32_t g = args.groups[static_cast<uint32_t>(args.sparse_keys[i])];
      if (g != NO_GROUP) {
         atomicAdd(&args.without_symbol[static_cast<size_t>(k) * args.n_groups + g], 1u);
      }
   }
}

/// A thread per (mutation, group).  A position with a derived symbol (LAYOUT_IMPLICIT) gives every row some symbol, so its
/// coverage is |filter ∩ range| less the rows without a valid symbol, and the derived symbol's count what the coverage leaves
/// after the stored symbols (the identity of k_finish_scan).  Elsewhere coverage = H_stored and count = H_sym.
__global__ __launch_bounds__(256) void k_finish_grouped(const GroupedArgs args, uint32_t* __restrict__ out) {
   const uint32_t i = blockIdx.x * 256u + threadIdx.x;
   if (i >= args.n_mutations * args.n_groups) {
      return;
   }
   const uint32_t m = i / args.n_groups;
   const uint32_t g = i % args.n_groups;
   const PositionLayout layout = layoutOf(args.dev, args.mut_position[m]);
   uint32_t count = args.h_sym[i];
   uint32_t coverage = args.h_stored[i];
   if (layout.implicit) {
      const uint32_t derived = args.mut_derived[m];
      const uint32_t without = derived != NO_POSITION ? args.without_symbol[static_cast<size_t>(derived) * args.n_groups + g] : 0u;
      coverage = args.cardinality[g] - without;
      if (codeOfSymbol(layout, args.mut_scan[m]) == CODE_IMPLICIT) {
         count = coverage - args.h_stored[i];
      }
   }
   out[2u * i] += count;  // launches into one table are ordered on the stream: no atomic needed
   out[2u * i + 1u] += coverage;
}

/// The filters of a K8 launch: filters[f] = a row bitset of row_words words, nullptr = all rows.
struct FilterCountArgs {
   const uint16_t* groups;          // [row_words * 64], as k_assign_groups left them
   const uint64_t* const* filters;  // [n_filters] (device array)
   uint32_t* out;                   // [n_filters][n_groups], accumulated into
   uint32_t row_words;
   uint32_t n_filters;
   uint32_t n_groups;
};

/// grid = (row_words / POSITION_THREADS rounded up, filter batches of FILTERS_PER_BLOCK); dynamic LDS: a histogram
/// [FILTERS_PER_BLOCK][n_groups].  A thread owns one row word: it decodes the 64 group ids once (decodeWordGroups), then per
/// filter of the batch splits the filter word by the (group, mask) pairs — row by row where the word has more groups than pairs.
/// A word without a row in any group reads no filter.  Rows past sequence_count have no group, so a filter's padding bits never
/// count.  One global add per non-zero entry at the end.
__global__ __launch_bounds__(POSITION_THREADS) void k_grouped_filter_counts(const FilterCountArgs args) {
   extern __shared__ uint32_t s_filter_hist[];  // [FILTERS_PER_BLOCK][n_groups]
   const uint32_t n_groups = args.n_groups;
   const uint32_t word = blockIdx.x * POSITION_THREADS + threadIdx.x;
   const bool has_word = word < args.row_words;
   const uint32_t f_begin = blockIdx.y * FILTERS_PER_BLOCK;
   const uint32_t batch = min(args.n_filters - f_begin, FILTERS_PER_BLOCK);  // (the grid has no block without a filter)
   for (uint32_t i = threadIdx.x; i < batch * n_groups; i += POSITION_THREADS) {
      s_filter_hist[i] = 0;
   }
   uint32_t seg_group[WORD_SEGMENTS];
   uint64_t seg_mask[WORD_SEGMENTS];
   const bool row_by_row = decodeWordGroups(args.groups, word, has_word, seg_group, seg_mask);
   __syncthreads();
   if (row_by_row || seg_mask[0] != 0) {  // (the first group met takes the first pair: none there = no row of the word in a group)
      for (uint32_t f = 0; f < batch; ++f) {
         const uint64_t* filter = args.filters[f_begin + f];  // (uniform)
         const uint64_t bits = filter != nullptr ? filter[word] : ~0ull;
         uint32_t* hist = s_filter_hist + f * n_groups;
         if (!row_by_row) {
#pragma unroll
            for (uint32_t s = 0; s < WORD_SEGMENTS; ++s) {
               const uint32_t count = static_cast<uint32_t>(__popcll(bits & seg_mask[s]));
               if (count != 0) {
                  atomicAdd(hist + seg_group[s], count);
               }
            }
         } else {
            for (uint64_t rest = bits; rest != 0; rest &= rest - 1) {
               const uint32_t g = args.groups[static_cast<size_t>(word) * 64u + static_cast<uint32_t>(__builtin_ctzll(rest))];
               if (g != NO_GROUP) {
                  atomicAdd(hist + g, 1u);
               }
            }
         }
      }
   }
   __syncthreads();
   uint32_t* out = args.out + static_cast<size_t>(f_begin) * n_groups;
   for (uint32_t i = threadIdx.x; i < batch * n_groups; i += POSITION_THREADS) {
      const uint32_t count = s_filter_hist[i];
      if (count != 0) {
         atomicAdd(out + i, count);
      }
   }
}

/// The ranges in order of their start (`order`: request indices; a range's group is its request index); they must be disjoint
/// with both ends inclusive.  Returns what is wrong with them, nullptr if nothing.
const char* orderRanges(const uint32_t* range_bounds, uint32_t n_ranges, std::vector<uint32_t>& order) {
   order.resize(n_ranges);
   std::iota(order.begin(), order.end(), 0u);
   std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return range_bounds[2u * a] < range_bounds[2u * b]; });
   for (uint32_t k = 0; k < n_ranges; ++k) {
      const uint32_t from = range_bounds[2u * order[k]], to = range_bounds[2u * order[k] + 1u];
      if (from > to) {
         return "a date range ends before it starts";
      }
      if (k > 0 && from <= range_bounds[2u * order[k - 1] + 1u]) {
         return "date ranges overlap";
      }
   }
   return nullptr;
}

}  // namespace

extern "C" {

int silo_gpu_mutations_grouped(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint64_t* filter_dev, const uint32_t* date_column_dev, const uint32_t* range_bounds,
   uint32_t n_ranges, const uint32_t* positions, const uint32_t* symbols, uint32_t n_mutations, void* group_scratch_dev, uint32_t* out_dev,
   void* stream
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || date_column_dev == nullptr || group_scratch_dev == nullptr || out_dev == nullptr ||
       (n_ranges != 0 && range_bounds == nullptr) || (n_mutations != 0 && (positions == nullptr || symbols == nullptr))) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_grouped: bad arguments");
   }
   if (n_ranges > SILO_GPU_MAX_DATE_RANGES || n_mutations > SILO_GPU_MAX_GROUPED_MUTATIONS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_grouped: too many date ranges or mutations");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (dev.planes == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_grouped: the sequence store holds no sequences yet");
   }
   std::vector<uint32_t> order;
   if (const char* complaint = orderRanges(range_bounds, n_ranges, order); complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_mutations_grouped: ") + complaint);
   }
   std::vector<uint32_t> scan_index(n_mutations);
   for (uint32_t m = 0; m < n_mutations; ++m) {
      if (positions[m] >= dev.positions || symbols[m] >= dev.n_symbols || dev.kind[symbols[m]] != PLANE_SCAN) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_grouped: position out of bounds or not a valid mutation symbol");
      }
      scan_index[m] = dev.index[symbols[m]];
   }
   if (n_ranges == 0 || n_mutations == 0) {
      return SILO_GPU_OK;
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);

   // listed positions whose most numerous symbol is derived: they need the rows without a valid symbol
   const auto derivedAt = [&](uint32_t position) {
      return dev.code_map != nullptr && !seqstore.layout.code_map.empty() &&(seqstore.layout.code_map[static_cast<size_t>(position) * CODE_MAP_STRIDE] & LAYOUT_IMPLICIT) != 0;
   };
   std::vector<uint32_t> derived_positions;
   for (uint32_t m = 0; m < n_mutations; ++m) {
      if (derivedAt(positions[m])) {
         derived_positions.push_back(positions[m]);
      }
   }
   std::sort(derived_positions.begin(), derived_positions.end());
   derived_positions.erase(std::unique(derived_positions.begin(), derived_positions.end()), derived_positions.end());
   const auto n_derived = static_cast<uint32_t>(derived_positions.size());

   // scratch: group ids, then the host tables, then the counters (zeroed)
   const uint32_t M = n_mutations, G = n_ranges;
   std::vector<uint32_t> tables(static_cast<size_t>(4) * M + M + 2u * M + 3u * G, 0u);
   uint32_t* t_position = tables.data();
   uint32_t* t_scan = t_position + M;
   uint32_t* t_derived = t_scan + M;
   uint32_t* t_first = t_derived + M;
   uint32_t* t_derived_positions = t_first + M;
   uint32_t* t_sparse = t_derived_positions + M;
   uint32_t* t_from = t_sparse + 2u * M;
   uint32_t* t_to = t_from + G;
   uint32_t* t_group = t_to + G;
   std::vector<bool> extra_counted(n_derived, false);
   for (uint32_t m = 0; m < M; ++m) {
      t_position[m] = positions[m];
      t_scan[m] = scan_index[m];
      t_derived[m] = NO_POSITION;
      if (derivedAt(positions[m])) {
         const auto k = static_cast<uint32_t>(std::lower_bound(derived_positions.begin(), derived_positions.end(), positions[m]) - derived_positions.begin());
         t_derived[m] = k;
         t_first[m] = extra_counted[k] ? 0u : 1u;
         extra_counted[k] = true;
      }
   }
   for (uint32_t k = 0; k < n_derived; ++k) {
      t_derived_positions[k] = derived_positions[k];
      const uint64_t first_key = static_cast<uint64_t>(derived_positions[k]) << 37;
      const auto lo = std::lower_bound(seqstore.sparse_sorted.begin(), seqstore.sparse_sorted.end(), first_key);
      const auto hi = std::lower_bound(lo, seqstore.sparse_sorted.end(), first_key + (uint64_t{1} << 37));
      t_sparse[2u * k] = static_cast<uint32_t>(lo - seqstore.sparse_sorted.begin());
      t_sparse[2u * k + 1u] = static_cast<uint32_t>(hi - seqstore.sparse_sorted.begin());
   }
   for (uint32_t k = 0; k < G; ++k) {
      t_from[k] = std::max<uint32_t>(range_bounds[2u * order[k]], 1u);
      t_to[k] = range_bounds[2u * order[k] + 1u];
      t_group[k] = order[k];
   }
   auto* base = static_cast<uint8_t*>(group_scratch_dev);
   const size_t group_bytes = static_cast<size_t>(dev.row_words) * 64u * sizeof(uint16_t);
   const size_t table_bytes = align256(tables.size() * sizeof(uint32_t));
   auto* d_tables = reinterpret_cast<uint32_t*>(base + group_bytes);
   auto* d_counters = reinterpret_cast<uint32_t*>(base + group_bytes + table_bytes);
   const size_t counter_words = static_cast<size_t>(G) + 2u * static_cast<size_t>(M) * G + static_cast<size_t>(n_derived) * G;
   if (group_bytes + table_bytes + counter_words * sizeof(uint32_t) > SILO_GPU_GROUPED_SCRATCH_BYTES(dev.row_words, n_ranges, n_mutations)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_grouped: scratch layout exceeds its documented size");  // (cannot happen)
   }
   HIP_TRY(hipMemcpyAsync(d_tables, tables.data(), tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipMemsetAsync(d_counters, 0, counter_words * sizeof(uint32_t), hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   GroupedArgs args{};
   args.dev = dev;
   args.groups = reinterpret_cast<uint16_t*>(base);
   args.mut_position = d_tables;
   args.mut_scan = d_tables + M;
   args.mut_derived = d_tables + 2u * M;
   args.mut_first = d_tables + 3u * M;
   args.derived_positions = d_tables + 4u * M;
   args.sparse_range = d_tables + 5u * M;
   args.bound_from = d_tables + 7u * M;
   args.bound_to = args.bound_from + G;
   args.bound_group = args.bound_to + G;
   args.cardinality = d_counters;
   args.h_sym = d_counters + G;
   args.h_stored = args.h_sym + static_cast<size_t>(M) * G;
   args.without_symbol = args.h_stored + static_cast<size_t>(M) * G;
   args.sparse_keys = seqstore.d_sparse.get();
   args.n_mutations = M;
   args.n_groups = G;
   args.n_derived = n_derived;
   args.sequence_count = store->sequence_count;
   if (dev.extra != nullptr) {
      for (uint32_t s = 0; s < dev.n_symbols; ++s) {
         if (dev.kind[s] == PLANE_EXTRA && args.n_extra < MAX_EXTRA) {
            args.extra_symbols[args.n_extra++] = static_cast<uint8_t>(s);
         }
      }
   }

   const uint32_t rows = dev.row_words * 64u;  // a multiple of GROUP_THREADS (rows are whole 256-byte lines)
   k_assign_groups<<<rows / GROUP_THREADS, GROUP_THREADS, 0, hip_stream>>>(args, filter_dev, date_column_dev);
   HIP_TRY(hipGetLastError());
   const dim3 position_grid((dev.row_words + POSITION_THREADS - 1) / POSITION_THREADS, (M + MUTATIONS_PER_BLOCK - 1) / MUTATIONS_PER_BLOCK);
   k_grouped_position_counts<<<position_grid, POSITION_THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   if (dev.escape_first != nullptr) {
      k_grouped_escapes<<<dim3(M, 4), 256, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (n_derived != 0) {
      if (dev.kind[dev.missing_symbol] == PLANE_RUNS && dev.n_missing_runs != 0) {
         const uint32_t blocks = std::min<uint32_t>((dev.n_missing_runs + 255u) / 256u, 2048u);
         k_grouped_missing_runs<<<blocks, 256, 0, hip_stream>>>(args);
         HIP_TRY(hipGetLastError());
      }
      if (!seqstore.sparse_sorted.empty()) {
         k_grouped_sparse_keys<<<dim3(n_derived, 4), 256, 0, hip_stream>>>(args);
         HIP_TRY(hipGetLastError());
      }
   }
   const size_t cells = static_cast<size_t>(M) * G;
   k_finish_grouped<<<static_cast<uint32_t>((cells + 255u) / 256u), 256, 0, hip_stream>>>(args, out_dev);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_filters_grouped(
   const silo_gpu_store* store, const uint64_t* base_filter_dev, const uint32_t* date_column_dev, const uint32_t* range_bounds, uint32_t n_ranges,
   const uint64_t* const* filters_dev, uint32_t n_filters, void* scratch_dev, uint32_t* out_dev, void* stream
) {
   if (store == nullptr || date_column_dev == nullptr || scratch_dev == nullptr || out_dev == nullptr || filters_dev == nullptr ||
       (n_ranges != 0 && range_bounds == nullptr)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_grouped: bad arguments");
   }
   if (n_ranges > SILO_GPU_MAX_DATE_RANGES || n_filters > SILO_GPU_MAX_GROUPED_FILTERS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_grouped: too many date ranges or filters");
   }
   if (store->sequence_count == 0 || store->row_words == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_grouped: the store has no rows");
   }
   std::vector<uint32_t> order;
   if (const char* complaint = orderRanges(range_bounds, n_ranges, order); complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_filters_grouped: ") + complaint);
   }
   if (n_ranges == 0 || n_filters == 0) {
      return SILO_GPU_OK;
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);

   // scratch: group ids, then the host tables (filter pointers, sorted bounds), then |base ∩ range| per group (zeroed)
   const uint32_t F = n_filters, G = n_ranges;
   std::vector<uint64_t> tables(static_cast<size_t>(F) + (3u * static_cast<size_t>(G) + 1u) / 2u, 0u);
   for (uint32_t f = 0; f < F; ++f) {
      tables[f] = reinterpret_cast<uint64_t>(filters_dev[f]);
   }
   auto* t_from = reinterpret_cast<uint32_t*>(tables.data() + F);
   uint32_t* t_to = t_from + G;
   uint32_t* t_group = t_to + G;
   for (uint32_t k = 0; k < G; ++k) {
      t_from[k] = std::max<uint32_t>(range_bounds[2u * order[k]], 1u);
      t_to[k] = range_bounds[2u * order[k] + 1u];
      t_group[k] = order[k];
   }
   auto* base = static_cast<uint8_t*>(scratch_dev);
   const size_t group_bytes = static_cast<size_t>(store->row_words) * 64u * sizeof(uint16_t);
   const size_t table_bytes = align256(tables.size() * sizeof(uint64_t));
   auto* d_tables = reinterpret_cast<uint64_t*>(base + group_bytes);
   auto* d_cardinality = reinterpret_cast<uint32_t*>(base + group_bytes + table_bytes);
   if (group_bytes + table_bytes + G * sizeof(uint32_t) > SILO_GPU_FILTERS_GROUPED_SCRATCH_BYTES(store->row_words, n_ranges, n_filters)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_grouped: scratch layout exceeds its documented size");  // (cannot happen)
   }
   HIP_TRY(hipMemcpyAsync(d_tables, tables.data(), tables.size() * sizeof(uint64_t), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipMemsetAsync(d_cardinality, 0, G * sizeof(uint32_t), hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   GroupedArgs args{};  // what k_assign_groups reads
   args.groups = reinterpret_cast<uint16_t*>(base);
   args.bound_from = reinterpret_cast<const uint32_t*>(d_tables + F);
   args.bound_to = args.bound_from + G;
   args.bound_group = args.bound_to + G;
   args.cardinality = d_cardinality;
   args.n_groups = G;
   args.sequence_count = store->sequence_count;
   const uint32_t rows = store->row_words * 64u;  // a multiple of GROUP_THREADS (rows are whole 256-byte lines)
   k_assign_groups<<<rows / GROUP_THREADS, GROUP_THREADS, 0, hip_stream>>>(args, base_filter_dev, date_column_dev);
   HIP_TRY(hipGetLastError());

   FilterCountArgs count_args{};
   count_args.groups = args.groups;
   count_args.filters = reinterpret_cast<const uint64_t* const*>(d_tables);
   count_args.out = out_dev;
   count_args.row_words = store->row_words;
   count_args.n_filters = F;
   count_args.n_groups = G;
   const dim3 grid((store->row_words + POSITION_THREADS - 1) / POSITION_THREADS, (F + FILTERS_PER_BLOCK - 1) / FILTERS_PER_BLOCK);
   const size_t lds_bytes = static_cast<size_t>(std::min(F, FILTERS_PER_BLOCK)) * G * sizeof(uint32_t);  // <= 32 KiB
   k_grouped_filter_counts<<<grid, POSITION_THREADS, lds_bytes, hip_stream>>>(count_args);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
