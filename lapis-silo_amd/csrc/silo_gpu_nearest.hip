// silo_gpu_nearest.hip — the nearest neighbours of a query over the whole store (K11).
//
// silo_gpu_query_distances: for every row of a sequence store the positions where both the query and the row hold a valid mutation
// symbol (compared) and where those two symbols differ (distance) — the two numbers silo_gpu_distance_pairs gives for the pair
// (query, row), but read off the adaptive layouts, one pass per kind of stored thing (the decomposition of K7, counted per row over
// all positions instead of per position over groups of rows):
//   k_query_init          every row's cell: the constants of the derived positions (every row agrees with the derived symbol until
//                         something stored says otherwise); (0, 0) for the padding rows
//   k_query_planes        the plane rows — the hot path: a thread owns one row word and walks a chunk of positions, adding the
//                         masks of each position into bit-sliced vertical counters in registers
//   k_query_escapes       a thread per escape key of the canonical position-major list
//   k_query_missing_runs  a thread per run of the missing symbol: two prefix lookups
//   k_query_sparse_keys   a thread per sparse key (ambiguity code)
// silo_gpu_nearest_rows: the k smallest (distance, row) of such a table under a filter.  (distance, row) is one integer key that no
// two rows share, so the k-th smallest key is found exactly by a radix select (k_nearest_histogram / k_nearest_pick per digit) and
// the rows at or below it are exactly the answer, ties at the k-th distance broken by the lowest row ids:
//   k_nearest_compact     appends them in any order
//   k_nearest_finish      one block sorts the <= SILO_GPU_MAX_NEAREST_ROWS keys and writes the list
// silo_gpu_bitset_from_distances: the rows of such a table within a distance of the query, as a row bitset (the filter expression
// WithinDistance):
//   k_bitset_from_distances  a thread per row, a wave's ballot per word
#include <algorithm>
#include <cstring>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t QUERY_THREADS = 256;  // one row word per thread: a block of k_query_planes covers 16 384 rows
// planes of a vertical counter.  Four counters of 12 planes are 96 VGPRs; an add ends at the first plane without a carry, so the
// width costs registers, not time.  A counter is unpacked once per 4 095 adds: 64 rows x 4 counters x 12 bit tests, ~1.5 operations
// per position — at 8 planes the unpacking would cost as much as the adds, 16 planes buy nothing but 32 more registers.
constexpr uint32_t COUNTER_PLANES = SILO_GPU_QUERY_DISTANCE_COUNTER_PLANES;
constexpr uint32_t COUNTER_MAX_ADDS = (1u << COUNTER_PLANES) - 1u;
constexpr uint32_t PLANE_PASS_BLOCKS = 2048;  // blocks the plane pass aims for: position chunks make up for few row words ...
// ... but a chunk is at least one counter's lifetime: unpacking (and the 128 adds to memory that follow) is then paid once per as
// many positions as a counter holds, wherever a chunk ends
constexpr uint32_t MIN_POSITION_CHUNK = 1u << COUNTER_PLANES;
constexpr uint32_t MAX_EXTRA = 16;
constexpr uint8_t NOT_VALID = 0xFF;

/// The valid mutation symbols as characters, exactly the ones silo_gpu_distance_pack compares.
constexpr const char* NUCLEOTIDE_VALID = "-ACGT";
constexpr const char* AMINO_ACID_VALID = "-ACDEFGHIKLMNPQRSTVWY*";

struct QueryArgs {
   SeqStoreDev dev;
   const uint8_t* q_scan;    // [P] scan symbol index of the query's character, NOT_VALID
   const uint32_t* pref_q;   // [P + 1] derived positions before p where the query is valid
   const uint32_t* pref_m;   // [P + 1] ... where it also differs from the derived symbol
   const uint64_t* sparse_keys;
   uint32_t n_sparse;
   uint32_t n_escapes;
   uint32_t sequence_count;
   uint32_t chunk;           // positions a block of k_query_planes walks
   uint32_t n_extra;
   uint8_t extra_symbols[MAX_EXTRA];  // symbols kept in extra planes (none of them a valid symbol)
   uint32_t* out;            // [row_words * 64][2] = distance, compared
};

/// A thread per row (the grid is exact: rows are whole 256-byte lines).
__global__ __launch_bounds__(QUERY_THREADS) void k_query_init(const QueryArgs args) {
   const uint32_t row = blockIdx.x * QUERY_THREADS + threadIdx.x;
   const uint32_t positions = args.dev.positions;
   const bool real = row < args.sequence_count;
   reinterpret_cast<uint2*>(args.out)[row] = real ? make_uint2(args.pref_m[positions], args.pref_q[positions]) : make_uint2(0u, 0u);
}

/// Adds the rows of `mask` to a vertical counter: a ripple-carry add that ends at the first plane no lane of the wave carries into.
__device__ __forceinline__ void counterAdd(uint64_t (&planes)[COUNTER_PLANES], uint64_t mask) {
#pragma unroll
   for (uint32_t k = 0; k < COUNTER_PLANES; ++k) {
      if (__ballot(mask != 0) == 0) {  // (uniform)
         break;
      }
      const uint64_t carry = planes[k] & mask;
      planes[k] ^= mask;
      mask = carry;
   }
}

__device__ __forceinline__ uint32_t counterOfRow(const uint64_t (&planes)[COUNTER_PLANES], uint32_t bit) {
   uint32_t value = 0;
#pragma unroll
   for (uint32_t k = 0; k < COUNTER_PLANES; ++k) {
      value |= static_cast<uint32_t>((planes[k] >> bit) & 1ull) << k;
   }
   return value;
}

__device__ __forceinline__ void counterClear(uint64_t (&planes)[COUNTER_PLANES]) {
#pragma unroll
   for (uint32_t k = 0; k < COUNTER_PLANES; ++k) {
      planes[k] = 0;
   }
}

/// grid = (row_words / QUERY_THREADS rounded up, position chunks).  A thread owns row word `word` and walks the positions of its
/// chunk where the query is valid (position tables and layouts are uniform: scalar loads); the loads of a wave are consecutive
/// words of one plane row.  Four vertical counters — what is added to and taken from compared and distance — so that nothing is
/// decoded inside the loop; they are unpacked into the rows' cells before one could overflow and at the end of the chunk.
__global__ __launch_bounds__(QUERY_THREADS) void k_query_planes(const QueryArgs args) {
   const uint32_t row_words = args.dev.row_words;
   const uint32_t word = blockIdx.x * QUERY_THREADS + threadIdx.x;
   if (word >= row_words) {
      return;
   }
   const uint32_t p_begin = blockIdx.y * args.chunk;
   const uint32_t p_end = min(args.dev.positions, p_begin + args.chunk);
   uint64_t c_plus[COUNTER_PLANES], c_minus[COUNTER_PLANES], d_plus[COUNTER_PLANES], d_minus[COUNTER_PLANES];
   counterClear(c_plus);
   counterClear(c_minus);
   counterClear(d_plus);
   counterClear(d_minus);
   uint32_t adds = 0;  // an upper bound of what any of the four has taken since it was cleared
   const uint32_t adds_per_position = args.n_extra != 0 ? 2u : 1u;  // only the rows of an extra plane are a counter's second add
   const auto flush = [&]() {
      for (uint32_t bit = 0; bit < 64u; ++bit) {
         const uint32_t row = word * 64u + bit;
         if (row >= args.sequence_count) {
            break;  // padding rows keep (0, 0)
         }
         const uint32_t distance = counterOfRow(d_plus, bit) - counterOfRow(d_minus, bit);
         const uint32_t compared = counterOfRow(c_plus, bit) - counterOfRow(c_minus, bit);
         if (distance != 0) {
            atomicAdd(args.out + 2u * static_cast<size_t>(row), distance);
         }
         if (compared != 0) {
            atomicAdd(args.out + 2u * static_cast<size_t>(row) + 1u, compared);
         }
      }
      counterClear(c_plus);
      counterClear(c_minus);
      counterClear(d_plus);
      counterClear(d_minus);
      adds = 0;
   };
   for (uint32_t position = p_begin; position < p_end; ++position) {
      const uint32_t scan_index = args.q_scan[position];
      if (scan_index == NOT_VALID) {
         continue;  // (uniform) nothing is compared here
      }
      if (adds + adds_per_position > COUNTER_MAX_ADDS) {
         flush();
      }
      adds += adds_per_position;
      const PositionLayout layout = layoutOf(args.dev, position);
      const uint32_t code = codeOfSymbol(layout, scan_index);
      if (!layout.implicit) {
         uint64_t stored = 0;
         for (uint32_t plane = 0; plane < layout.bits; ++plane) {
            stored |= layout.rows[static_cast<size_t>(plane) * row_words + word];
         }
         const uint64_t same = code != CODE_ESCAPED ? decodeCodeWord(layout, row_words, code, word) : 0ull;
         counterAdd(c_plus, stored);
         counterAdd(d_plus, stored & ~same);
         continue;
      }
      // a derived position: every row was given the derived symbol by k_query_init; the one-hot rows say which have another
      if (code == CODE_IMPLICIT) {
         uint64_t stored = 0;
         for (uint32_t plane = 0; plane < layout.bits; ++plane) {
            stored |= layout.rows[static_cast<size_t>(plane) * row_words + word];
         }
         counterAdd(d_plus, stored);
      } else if (code != CODE_ESCAPED) {
         counterAdd(d_minus, layout.rows[static_cast<size_t>(code - 1u) * row_words + word]);
      }
      if (args.n_extra != 0) {  // rows without a valid symbol that sit in a plane of their own
         uint64_t none = 0;
         for (uint32_t e = 0; e < args.n_extra; ++e) {
            none |= planePtr(args.dev, position, args.extra_symbols[e])[word];
         }
         counterAdd(c_minus, none);
         if (code != CODE_IMPLICIT) {
            counterAdd(d_minus, none);
         }
      }
   }
   if (adds != 0) {
      flush();
   }
}

/// A thread per escape key (grid-stride): a row's valid symbol that has neither a code nor a row at its position.
__global__ __launch_bounds__(256) void k_query_escapes(const QueryArgs args) {
   for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < args.n_escapes; i += gridDim.x * 256u) {
      const uint64_t key = args.dev.escapes[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      const uint32_t symbol = static_cast<uint32_t>(key >> 32) & 31u;
      const uint32_t row = static_cast<uint32_t>(key);
      if (position >= args.dev.positions || row >= args.sequence_count) {
         continue;
      }
      const uint32_t scan_index = args.q_scan[position];
      if (scan_index == NOT_VALID) {
         continue;
      }
      const uint8_t* map = args.dev.code_map + static_cast<size_t>(position) * CODE_MAP_STRIDE;
      uint32_t* cell = args.out + 2u * static_cast<size_t>(row);
      if ((map[0] & LAYOUT_IMPLICIT) == 0) {
         atomicAdd(cell + 1, 1u);
         if (symbol != scan_index) {
            atomicAdd(cell, 1u);
         }
      } else if (scan_index == map[IMPLICIT_SLOT]) {
         atomicAdd(cell, 1u);  // counted as agreeing with the derived symbol
      } else if (scan_index == symbol) {
         atomicAdd(cell, 0xFFFFFFFFu);  // counted as differing from it
      }
   }
}

/// What a row without a valid symbol at the derived positions [from, to) takes back from the constants.
__device__ __forceinline__ void takeBack(const QueryArgs& args, uint32_t row, uint32_t from, uint32_t to) {
   if (row >= args.sequence_count) {
      return;
   }
   const uint32_t compared = args.pref_q[to] - args.pref_q[from];
   const uint32_t distance = args.pref_m[to] - args.pref_m[from];
   uint32_t* cell = args.out + 2u * static_cast<size_t>(row);
   if (distance != 0) {
      atomicAdd(cell, 0u - distance);
   }
   if (compared != 0) {
      atomicAdd(cell + 1, 0u - compared);
   }
}

/// A thread per run of the missing symbol (grid-stride).
__global__ __launch_bounds__(256) void k_query_missing_runs(const QueryArgs args) {
   for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < args.dev.n_missing_runs; i += gridDim.x * 256u) {
      const uint64_t key = args.dev.missing_run_keys[i];
      const uint32_t start = static_cast<uint32_t>(key);
      const uint32_t end = min(args.dev.missing_run_ends[i], args.dev.positions);
      if (start < end) {
         takeBack(args, static_cast<uint32_t>(key >> 32), start, end);
      }
   }
}

/// A thread per sparse key (grid-stride): an ambiguity code, or the missing symbol where it has neither runs nor a plane.
__global__ __launch_bounds__(256) void k_query_sparse_keys(const QueryArgs args) {
   for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < args.n_sparse; i += gridDim.x * 256u) {
      const uint64_t key = args.sparse_keys[i];
      const uint32_t position = static_cast<uint32_t>(key >> 37);
      if (position < args.dev.positions) {
         takeBack(args, static_cast<uint32_t>(key), position, position + 1u);
      }
   }
}

// ---- the k smallest -------------------------------------------------------------------------------------
constexpr uint32_t DIGIT_BITS = 12;
constexpr uint32_t DIGIT_BINS = 1u << DIGIT_BITS;  // 16 KiB of LDS
constexpr uint32_t SELECT_THREADS = 256;
constexpr uint32_t SELECT_MAX_BLOCKS = 1024;
constexpr uint32_t FINISH_THREADS = SILO_GPU_MAX_NEAREST_ROWS;
static_assert((FINISH_THREADS & (FINISH_THREADS - 1u)) == 0 && FINISH_THREADS <= 1024u);

/// The state of one selection, at the start of the scratch (zeroed by the entry point).
struct SelectState {
   unsigned long long prefix;  // the digits of the k-th smallest key found so far
   uint32_t remaining;         // its rank (1-based) among the eligible keys that share those digits
   uint32_t take_all;          // no more than k rows are eligible: all of them are the answer
   uint32_t n_candidates;      // appended by k_nearest_compact
};
constexpr size_t STATE_BYTES = 256;
constexpr size_t HISTOGRAM_BYTES = DIGIT_BINS * sizeof(uint32_t);
static_assert(sizeof(SelectState) <= STATE_BYTES);
static_assert(STATE_BYTES + HISTOGRAM_BYTES + SILO_GPU_MAX_NEAREST_ROWS * sizeof(uint64_t) <= SILO_GPU_NEAREST_ROWS_SCRATCH_BYTES);

struct SelectArgs {
   const uint32_t* table;   // [rows][2] = distance, compared
   const uint64_t* filter;  // nullptr = all rows
   SelectState* state;
   uint32_t* histogram;     // [DIGIT_BINS]
   unsigned long long* candidates;  // [SILO_GPU_MAX_NEAREST_ROWS]
   uint32_t sequence_count;
   uint32_t exclude_row;
   uint32_t max_distance;
   uint32_t k;
   uint32_t row_bits;       // key = distance << row_bits | row
};

/// The key of a row, and whether the row takes part at all.
__device__ __forceinline__ bool keyOfRow(const SelectArgs& args, uint32_t row, unsigned long long& key) {
   if (row >= args.sequence_count || row == args.exclude_row) {
      return false;  // (padding bits of a filter never select a row)
   }
   if (args.filter != nullptr && ((args.filter[row >> 6] >> (row & 63u)) & 1ull) == 0) {
      return false;
   }
   const uint32_t distance = args.table[2u * static_cast<size_t>(row)];
   key = (static_cast<unsigned long long>(distance) << args.row_bits) | row;
   return distance <= args.max_distance;
}

/// Grid-stride, a thread per row: the histogram of the digit at `shift` over the eligible keys that share the digits above it with
/// the prefix (`first`: over all eligible keys).  Block-private in LDS; a wave whose rows all fall in one bin — the high digits of
/// small distances — adds once.  Integer adds only: the histogram does not depend on the scheduling.
__global__ __launch_bounds__(SELECT_THREADS) void k_nearest_histogram(const SelectArgs args, uint32_t shift, bool first) {
   __shared__ uint32_t s_bins[DIGIT_BINS];
   for (uint32_t i = threadIdx.x; i < DIGIT_BINS; i += SELECT_THREADS) {
      s_bins[i] = 0;
   }
   __syncthreads();
   const bool idle = !first && args.state->take_all != 0;  // (uniform) nothing left to find
   const unsigned long long prefix = args.state->prefix;
   const uint32_t rows = (args.sequence_count + 63u) / 64u * 64u;
   for (uint32_t base = blockIdx.x * SELECT_THREADS; base < rows && !idle; base += gridDim.x * SELECT_THREADS) {
      unsigned long long key = 0;
      bool counts = keyOfRow(args, base + threadIdx.x, key);
      if (counts && !first) {
         counts = (key >> (shift + DIGIT_BITS)) == (prefix >> (shift + DIGIT_BITS));
      }
      if (counts) {
         const uint32_t digit = static_cast<uint32_t>(key >> shift) & (DIGIT_BINS - 1u);
         const uint32_t lead = __builtin_amdgcn_readfirstlane(digit);
         const uint64_t active = __ballot(true);
         if (__ballot(digit == lead) == active) {
            if ((threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(active))) {
               atomicAdd(&s_bins[lead], static_cast<uint32_t>(__popcll(active)));
            }
         } else {
            atomicAdd(&s_bins[digit], 1u);
         }
      }
   }
   __syncthreads();
   for (uint32_t i = threadIdx.x; i < DIGIT_BINS; i += SELECT_THREADS) {
      if (s_bins[i] != 0) {
         atomicAdd(&args.histogram[i], s_bins[i]);
      }
   }
}

/// One block: the digit at `shift` of the k-th smallest key from the histogram, which it clears for the next digit.
__global__ __launch_bounds__(SELECT_THREADS) void k_nearest_pick(const SelectArgs args, uint32_t shift, bool first) {
   constexpr uint32_t PER_THREAD = DIGIT_BINS / SELECT_THREADS;
   __shared__ uint32_t s_bins[DIGIT_BINS];
   __shared__ uint32_t s_partial[SELECT_THREADS];
   uint32_t partial = 0;
   for (uint32_t i = 0; i < PER_THREAD; ++i) {
      const uint32_t bin = threadIdx.x * PER_THREAD + i;
      const uint32_t count = args.histogram[bin];
      args.histogram[bin] = 0;
      s_bins[bin] = count;
      partial += count;
   }
   s_partial[threadIdx.x] = partial;
   __syncthreads();
   if (threadIdx.x != 0) {
      return;
   }
   SelectState& state = *args.state;
   if (first) {
      uint32_t total = 0;
      for (uint32_t t = 0; t < SELECT_THREADS; ++t) {
         total += s_partial[t];
      }
      state.take_all = total <= args.k ? 1u : 0u;
      state.remaining = args.k;
      state.prefix = 0;
   }
   if (state.take_all != 0) {
      return;
   }
   uint32_t remaining = state.remaining;  // >= 1 and <= the sum of the histogram
   uint32_t t = 0;
   while (t + 1u < SELECT_THREADS && s_partial[t] < remaining) {
      remaining -= s_partial[t++];
   }
   uint32_t bin = t * PER_THREAD;
   while (bin + 1u < (t + 1u) * PER_THREAD && s_bins[bin] < remaining) {
      remaining -= s_bins[bin++];
   }
   state.prefix |= static_cast<unsigned long long>(bin) << shift;
   state.remaining = remaining;
}

/// Grid-stride, a thread per row: the eligible rows at or below the k-th smallest key — exactly min(k, eligible) of them.
__global__ __launch_bounds__(SELECT_THREADS) void k_nearest_compact(const SelectArgs args) {
   const bool take_all = args.state->take_all != 0;
   const unsigned long long threshold = args.state->prefix;
   for (uint32_t row = blockIdx.x * SELECT_THREADS + threadIdx.x; row < args.sequence_count; row += gridDim.x * SELECT_THREADS) {
      unsigned long long key = 0;
      if (keyOfRow(args, row, key) && (take_all || key <= threshold)) {
         const uint32_t slot = atomicAdd(&args.state->n_candidates, 1u);
         if (slot < args.k) {
            args.candidates[slot] = key;
         }
      }
   }
}

/// One block: a bitonic sort of the candidates' keys in LDS, then the list.  The keys are distinct, so their order — and with it
/// the output — does not depend on the order they were appended in.
__global__ __launch_bounds__(FINISH_THREADS) void k_nearest_finish(const SelectArgs args, uint32_t* __restrict__ out, uint32_t* __restrict__ out_count) {
   __shared__ unsigned long long s_keys[FINISH_THREADS];
   const uint32_t count = min(args.state->n_candidates, args.k);
   s_keys[threadIdx.x] = threadIdx.x < count ? args.candidates[threadIdx.x] : ~0ull;
   __syncthreads();
   for (uint32_t size = 2; size <= FINISH_THREADS; size <<= 1) {
      for (uint32_t stride = size >> 1; stride != 0; stride >>= 1) {
         const uint32_t partner = threadIdx.x ^ stride;
         if (partner > threadIdx.x) {
            const bool ascending = (threadIdx.x & size) == 0;
            const unsigned long long mine = s_keys[threadIdx.x], other = s_keys[partner];
            if ((mine > other) == ascending) {
               s_keys[threadIdx.x] = other;
               s_keys[partner] = mine;
            }
         }
         __syncthreads();
      }
   }
   if (threadIdx.x < count) {
      const unsigned long long key = s_keys[threadIdx.x];
      const uint32_t row = static_cast<uint32_t>(key & ((1ull << args.row_bits) - 1ull));
      out[3u * threadIdx.x] = row;
      out[3u * threadIdx.x + 1u] = static_cast<uint32_t>(key >> args.row_bits);
      out[3u * threadIdx.x + 2u] = args.table[2u * static_cast<size_t>(row) + 1u];
   }
   if (threadIdx.x == 0) {
      *out_count = count;
   }
}

// ---- the rows within a distance -------------------------------------------------------------------------
constexpr uint32_t BITSET_THREADS = 256;  // four waves, four output words
static_assert(BITSET_THREADS % 64u == 0);

/// A thread per row of the table, a wave per word of the bitset: one 8-byte load per lane (a wave reads 512 consecutive bytes), the
/// wave's ballot of the predicate is the word, stored by its first lane.  A wave whose word is at or past row_words neither loads
/// nor stores (the grid is rounded up to whole blocks); rows at or past sequence_count give 0 whatever their cell holds.
__global__ __launch_bounds__(BITSET_THREADS) void k_bitset_from_distances(
   const uint2* __restrict__ table, uint32_t sequence_count, uint32_t row_words, uint32_t max_distance, uint32_t min_compared,
   uint64_t* __restrict__ out
) {
   const size_t row = static_cast<size_t>(blockIdx.x) * BITSET_THREADS + threadIdx.x;
   const size_t word = row >> 6;  // (uniform over the wave)
   if (word >= row_words) {
      return;
   }
   const uint2 cell = table[row];  // .x = distance, .y = compared
   const bool selected = row < sequence_count && cell.x <= max_distance && cell.y >= min_compared;
   const uint64_t bits = __ballot(selected);
   if ((threadIdx.x & 63u) == 0) {
      out[word] = bits;
   }
}

}  // namespace

extern "C" {

int silo_gpu_bitset_from_distances(
   const uint32_t* table_dev, uint32_t sequence_count, uint32_t row_words, uint32_t max_distance, uint32_t min_compared, uint64_t* out_bitset_dev,
   void* stream
) {
   if (table_dev == nullptr || out_bitset_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_from_distances: bad arguments");
   }
   if (row_words == 0 || sequence_count == 0 || sequence_count > static_cast<uint64_t>(row_words) * 64u) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_bitset_from_distances: the table has no rows, or fewer than sequence_count");
   }
   constexpr uint32_t WORDS_PER_BLOCK = BITSET_THREADS / 64u;
   const uint32_t blocks = row_words / WORDS_PER_BLOCK + (row_words % WORDS_PER_BLOCK != 0 ? 1u : 0u);
   k_bitset_from_distances<<<blocks, BITSET_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const uint2*>(table_dev), sequence_count, row_words, max_distance, min_compared, out_bitset_dev
   );
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_query_distances(
   const silo_gpu_store* store, uint32_t seqstore_id, const char* query_chars, uint32_t* out_dev, void* scratch_dev, void* stream
) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || query_chars == nullptr || out_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_query_distances: bad arguments");
   }
   const SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   const SeqStoreDev& dev = seqstore.dev;
   if (dev.planes == nullptr || store->sequence_count == 0 || dev.row_words == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_query_distances: the sequence store holds no sequences yet");
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);
   const uint32_t P = dev.positions;

   // the per-position tables: the query as scan symbol indices, the two prefix counts over the derived positions
   uint8_t char_table[256];
   fillCharTable(seqstore.alphabet, char_table);
   uint8_t scan_of_char[256];
   memset(scan_of_char, NOT_VALID, sizeof(scan_of_char));
   for (const char* c = seqstore.alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE ? NUCLEOTIDE_VALID : AMINO_ACID_VALID; *c != 0; ++c) {
      const uint8_t symbol = char_table[static_cast<uint8_t>(*c)];
      if (symbol < dev.n_symbols && dev.kind[symbol] == PLANE_SCAN) {
         scan_of_char[static_cast<uint8_t>(*c)] = dev.index[symbol];
      }
   }
   const bool has_map = dev.code_map != nullptr && !seqstore.layout.code_map.empty();
   const size_t scan_bytes = align256(P);
   const size_t prefix_bytes = align256((static_cast<size_t>(P) + 1u) * sizeof(uint32_t));
   if (scan_bytes + 2u * prefix_bytes > SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES(P)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_query_distances: scratch layout exceeds its documented size");  // (cannot happen)
   }
   std::vector<uint8_t> tables(scan_bytes + 2u * prefix_bytes, 0);
   uint8_t* t_scan = tables.data();
   auto* t_pref_q = reinterpret_cast<uint32_t*>(tables.data() + scan_bytes);
   auto* t_pref_m = reinterpret_cast<uint32_t*>(tables.data() + scan_bytes + prefix_bytes);
   for (uint32_t p = 0; p < P; ++p) {
      const uint8_t scan_index = scan_of_char[static_cast<uint8_t>(query_chars[p])];
      t_scan[p] = scan_index;
      const uint8_t* map = has_map ? seqstore.layout.code_map.data() + static_cast<size_t>(p) * CODE_MAP_STRIDE : nullptr;
      const bool derived = map != nullptr && (map[0] & LAYOUT_IMPLICIT) != 0 && scan_index != NOT_VALID;
      t_pref_q[p + 1u] = t_pref_q[p] + (derived ? 1u : 0u);
      t_pref_m[p + 1u] = t_pref_m[p] + (derived && map[IMPLICIT_SLOT] != scan_index ? 1u : 0u);
   }
   auto* base = static_cast<uint8_t*>(scratch_dev);
   HIP_TRY(hipMemcpyAsync(base, tables.data(), tables.size(), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   QueryArgs args{};
   args.dev = dev;
   args.q_scan = base;
   args.pref_q = reinterpret_cast<const uint32_t*>(base + scan_bytes);
   args.pref_m = reinterpret_cast<const uint32_t*>(base + scan_bytes + prefix_bytes);
   args.sparse_keys = seqstore.d_sparse.get();
   args.n_sparse = seqstore.d_sparse.get() != nullptr ? static_cast<uint32_t>(seqstore.sparse_sorted.size()) : 0u;
   args.n_escapes = has_map && dev.escapes != nullptr && dev.escape_first != nullptr && !seqstore.layout.escape_first.empty()
                       ? seqstore.layout.escape_first.back()
                       : 0u;
   args.sequence_count = store->sequence_count;
   args.out = out_dev;
   if (dev.extra != nullptr) {
      for (uint32_t s = 0; s < dev.n_symbols; ++s) {
         if (dev.kind[s] == PLANE_EXTRA && args.n_extra < MAX_EXTRA) {
            args.extra_symbols[args.n_extra++] = static_cast<uint8_t>(s);
         }
      }
   }
   const uint32_t word_blocks = (dev.row_words + QUERY_THREADS - 1) / QUERY_THREADS;
   const uint32_t wanted_chunks = std::max<uint32_t>(1u, PLANE_PASS_BLOCKS / word_blocks);
   args.chunk = std::max<uint32_t>(MIN_POSITION_CHUNK, (P + wanted_chunks - 1) / wanted_chunks);
   const uint32_t chunks = std::max<uint32_t>(1u, (P + args.chunk - 1) / args.chunk);

   const uint32_t rows = dev.row_words * 64u;  // a multiple of QUERY_THREADS (rows are whole 256-byte lines)
   k_query_init<<<rows / QUERY_THREADS, QUERY_THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   if (P != 0) {
      k_query_planes<<<dim3(word_blocks, chunks), QUERY_THREADS, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (args.n_escapes != 0) {
      k_query_escapes<<<strideBlocks(args.n_escapes, 256u), 256, 0, hip_stream>>>(args);
      HIP_TRY(hipGetLastError());
   }
   if (t_pref_q[P] != 0) {  // only derived positions have rows to take back
      if (dev.kind[dev.missing_symbol] == PLANE_RUNS && dev.n_missing_runs != 0) {
         k_query_missing_runs<<<strideBlocks(dev.n_missing_runs, 256u), 256, 0, hip_stream>>>(args);
         HIP_TRY(hipGetLastError());
      }
      if (args.n_sparse != 0) {
         k_query_sparse_keys<<<strideBlocks(args.n_sparse, 256u), 256, 0, hip_stream>>>(args);
         HIP_TRY(hipGetLastError());
      }
   }
   return SILO_GPU_OK;
}

int silo_gpu_nearest_rows(
   const uint32_t* table_dev, const uint64_t* filter_dev, uint32_t sequence_count, uint32_t exclude_row, uint32_t max_distance, uint32_t k,
   uint32_t* out_dev, uint32_t* out_count_dev, void* scratch_dev, void* stream
) {
   if (table_dev == nullptr || out_dev == nullptr || out_count_dev == nullptr || scratch_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_rows: bad arguments");
   }
   if (k == 0 || k > SILO_GPU_MAX_NEAREST_ROWS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_rows: k is 0 or above SILO_GPU_MAX_NEAREST_ROWS");
   }
   if (sequence_count == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_nearest_rows: the table has no rows");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   auto* base = static_cast<uint8_t*>(scratch_dev);
   HIP_TRY(hipMemsetAsync(base, 0, STATE_BYTES + HISTOGRAM_BYTES, hip_stream));

   SelectArgs args{};
   args.table = table_dev;
   args.filter = filter_dev;
   args.state = reinterpret_cast<SelectState*>(base);
   args.histogram = reinterpret_cast<uint32_t*>(base + STATE_BYTES);
   args.candidates = reinterpret_cast<unsigned long long*>(base + STATE_BYTES + HISTOGRAM_BYTES);
   args.sequence_count = sequence_count;
   args.exclude_row = exclude_row;
   args.max_distance = max_distance;
   args.k = k;
   args.row_bits = 1;
   while (args.row_bits < 32u && (1ull << args.row_bits) < sequence_count) {
      ++args.row_bits;
   }
   const uint32_t key_bits = 32u + args.row_bits;
   const uint32_t digits = (key_bits + DIGIT_BITS - 1) / DIGIT_BITS;
   const uint32_t blocks = std::min<uint32_t>((sequence_count + SELECT_THREADS - 1) / SELECT_THREADS, SELECT_MAX_BLOCKS);
   for (uint32_t digit = 0; digit < digits; ++digit) {  // from the most significant digit down
      const uint32_t shift = (digits - 1u - digit) * DIGIT_BITS;
      k_nearest_histogram<<<blocks, SELECT_THREADS, 0, hip_stream>>>(args, shift, digit == 0);
      HIP_TRY(hipGetLastError());
      k_nearest_pick<<<1, SELECT_THREADS, 0, hip_stream>>>(args, shift, digit == 0);
      HIP_TRY(hipGetLastError());
   }
   k_nearest_compact<<<blocks, SELECT_THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   k_nearest_finish<<<1, FINISH_THREADS, 0, hip_stream>>>(args, out_dev, out_count_dev);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
