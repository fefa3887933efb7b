// silo_gpu_compare.hip — K17, the comparison of count tables behind MutationsComparison / AminoAcidMutationsComparison (DESIGN.md
// §24): for 2 .. 64 count tables as a Mutations scan leaves them — counts[table][position][valid symbol] — the cells (position,
// symbol) that some table passes at minProportion and whose proportions differ by at least minDifference between the tables, as a
// compact list with every table's count and coverage.  Takes no store.
//
// Kernel:
//   k_mutations_compare<N>   a block per 256 positions, a thread per position: a sweep over the tables, each table's slab of the
//                            block through LDS with 16-byte loads, the pass mask and the running max / min proportion of every
//                            symbol in registers; one integer add per thread for its slots; a second sweep over the thread's own
//                            cells for the count / coverage pairs of its records (silo_gpu_mutations_compare)
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t COMPARE_THREADS = SILO_GPU_COMPARE_THREADS;
constexpr uint32_t NUC_VALID = 5;   // "-ACGT"
constexpr uint32_t AA_VALID = 22;   // "-ACDEFGHIKLMNPQRSTVWY*"
constexpr uint32_t HEADER_WORDS = 4;

/// Two words of the output written together: a record {position, symbol} or a cell {count, coverage}.
struct WordPair {
   uint32_t first;
   uint32_t second;
};

/// grid = ceil(n_positions / 256); block x owns positions [256 x, 256 x + owned), thread i position 256 x + i.
/// First sweep, a rolled loop over the tables: the owned * N words of the block in table t are contiguous; they start at any
/// multiple of 4 bytes, so the block loads the 16-byte quads that cover them — a quad that would reach outside the n_tables tables
/// is loaded word by word, inside only — into LDS (as k_consensus_call stages its one slab), where a thread finds its N words at a
/// stride of N.  Per table the coverage = sum of the N counts and, where it is above 0, K4's bound (k_mutations_select: IEEE
/// double product, ceil, minus one, then integers); per symbol the pass bit, and the highest and lowest proportion (IEEE double
/// division) over the covered tables.  `c`, `highest` and `lowest` are indexed by unrolled constants only (no scratch).
/// Selection: symbol s of the position is selected iff it is not the reference's, some table passes it and highest - lowest >=
/// min_difference (0.0 where one table is covered: then highest == lowest).  A thread takes popc(selected) slots with ONE integer
/// atomicAdd on the header's counter — past `capacity` only the counter advances — and writes {position, symbol} of those that fit.
/// Second sweep: the thread re-reads its own N words of every table from global memory (read a moment ago: L2) and writes {count,
/// coverage} of table t for record slot i at cells[(i * n_tables + t) * 2].  Nothing read from a table or from the reference index
/// is used as an index.
template <uint32_t N>
__global__ __launch_bounds__(COMPARE_THREADS) void k_mutations_compare(
   const uint32_t* __restrict__ counts, uint32_t n_tables, uint32_t n_positions, const uint8_t* __restrict__ reference_index, double min_proportion,
   double min_difference, uint32_t capacity, uint32_t* __restrict__ out
) {
   __shared__ __attribute__((aligned(16))) uint32_t s_slab[COMPARE_THREADS * N + 4u];
   const uint32_t first = blockIdx.x * COMPARE_THREADS;
   const uint32_t owned = min(COMPARE_THREADS, n_positions - first);
   const uint32_t position = first + threadIdx.x;
   const bool mine = threadIdx.x < owned;
   const size_t table_words = static_cast<size_t>(n_positions) * N;
   const auto all_words = static_cast<int64_t>(table_words * n_tables);

   uint32_t passes = 0;   // bit s: some table passes symbol s
   double highest[N];
   double lowest[N];
#pragma unroll
   for (uint32_t s = 0; s < N; ++s) {
      highest[s] = 0.0;
      lowest[s] = 1.0;
   }
   for (uint32_t table = 0; table < n_tables; ++table) {
      const auto slab_begin = static_cast<int64_t>(table * table_words + static_cast<size_t>(first) * N);  // word of counts
      const uint32_t* slab = counts + slab_begin;
      const auto lead = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(slab) >> 2) & 3u);  // words from the 16-byte boundary below
      const uint32_t* aligned = slab - lead;
      const uint32_t quads = (lead + owned * N + 3u) / 4u;
      for (uint32_t quad = threadIdx.x; quad < quads; quad += COMPARE_THREADS) {
         const int64_t word = slab_begin - lead + static_cast<int64_t>(quad) * 4;  // of counts; below 0 or past the end: not ours to read
         if (word >= 0 && word + 4 <= all_words) {
            *reinterpret_cast<uint4*>(s_slab + quad * 4u) = *reinterpret_cast<const uint4*>(aligned + quad * 4u);
         } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
               if (word + k >= 0 && word + k < all_words) {
                  s_slab[quad * 4u + k] = aligned[quad * 4u + k];
               }
            }
         }
      }
      __syncthreads();
      if (mine) {
         uint32_t c[N];
         uint32_t coverage = 0;
#pragma unroll
         for (uint32_t s = 0; s < N; ++s) {
            c[s] = s_slab[lead + threadIdx.x * N + s];
            coverage += c[s];
         }
         if (coverage != 0) {
            const uint32_t bound = min_proportion == 0 ? 0u : static_cast<uint32_t>(ceil(static_cast<double>(coverage) * min_proportion) - 1);
            const auto total = static_cast<double>(coverage);
#pragma unroll
            for (uint32_t s = 0; s < N; ++s) {
               passes |= (c[s] > bound ? 1u : 0u) << s;
               const double proportion = static_cast<double>(c[s]) / total;
               highest[s] = fmax(highest[s], proportion);
               lowest[s] = fmin(lowest[s], proportion);
            }
         }
      }
      __syncthreads();  // the slab is read: the next table may overwrite it
   }

   if (!mine || passes == 0) {
      return;
   }
   const uint32_t reference = reference_index[position];
   uint32_t selected = 0;  // bit s: symbol s is a record
#pragma unroll
   for (uint32_t s = 0; s < N; ++s) {
      const double difference = highest[s] - lowest[s];  // over the covered tables, of which a pass needs one
      if (s != reference && ((passes >> s) & 1u) != 0 && difference >= min_difference) {
         selected |= 1u << s;
      }
   }
   if (selected == 0) {
      return;
   }
   const uint32_t slot = atomicAdd(&out[0], static_cast<uint32_t>(__popc(selected)));
   if (slot >= capacity) {
      return;
   }
   auto* records = reinterpret_cast<WordPair*>(out + HEADER_WORDS);
   auto* cells = reinterpret_cast<WordPair*>(out + HEADER_WORDS + static_cast<size_t>(capacity) * 2u);
   {
      uint32_t at = slot;
#pragma unroll
      for (uint32_t s = 0; s < N; ++s) {
         if (((selected >> s) & 1u) != 0) {
            if (at < capacity) {
               records[at] = WordPair{position, s};
            }
            ++at;
         }
      }
   }
   for (uint32_t table = 0; table < n_tables; ++table) {
      const uint32_t* at_position = counts + table * table_words + static_cast<size_t>(position) * N;
      uint32_t c[N];
      uint32_t coverage = 0;
#pragma unroll
      for (uint32_t s = 0; s < N; ++s) {
         c[s] = at_position[s];
         coverage += c[s];
      }
      uint32_t at = slot;
#pragma unroll
      for (uint32_t s = 0; s < N; ++s) {
         if (((selected >> s) & 1u) != 0) {
            if (at < capacity) {
               cells[static_cast<size_t>(at) * n_tables + table] = WordPair{c[s], coverage};
            }
            ++at;
         }
      }
   }
}

}  // namespace

extern "C" {

int silo_gpu_mutations_compare(
   int alphabet, const uint32_t* counts_dev, uint32_t n_tables, uint32_t n_positions, const uint8_t* reference_index_dev, double min_proportion,
   double min_difference, uint32_t capacity, uint32_t* out_dev, void* stream
) {
   if (alphabet != SILO_GPU_ALPHABET_NUCLEOTIDE && alphabet != SILO_GPU_ALPHABET_AMINO_ACID) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_compare: unknown alphabet");
   }
   if (counts_dev == nullptr || reference_index_dev == nullptr || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_compare: a buffer is NULL");
   }
   if (n_tables < 2 || n_tables > SILO_GPU_MAX_COMPARISON_TABLES) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_compare: the number of tables is not in [2, SILO_GPU_MAX_COMPARISON_TABLES]");
   }
   if (!(min_proportion >= 0.0 && min_proportion <= 1.0) || !(min_difference >= 0.0 && min_difference <= 1.0)) {  // (NaN fails both)
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_compare: min_proportion or min_difference is not in [0, 1]");
   }
   if ((reinterpret_cast<uintptr_t>(counts_dev) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_dev) & 3u) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_mutations_compare: the count tables or the output are not 4-byte aligned");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   HIP_TRY(hipMemsetAsync(out_dev, 0, HEADER_WORDS * sizeof(uint32_t), hip_stream));
   if (n_positions == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t blocks = (n_positions + COMPARE_THREADS - 1u) / COMPARE_THREADS;
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_mutations_compare<NUC_VALID><<<blocks, COMPARE_THREADS, 0, hip_stream>>>(
         counts_dev, n_tables, n_positions, reference_index_dev, min_proportion, min_difference, capacity, out_dev
      );
   } else {
      k_mutations_compare<AA_VALID><<<blocks, COMPARE_THREADS, 0, hip_stream>>>(
         counts_dev, n_tables, n_positions, reference_index_dev, min_proportion, min_difference, capacity, out_dev
      );
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
