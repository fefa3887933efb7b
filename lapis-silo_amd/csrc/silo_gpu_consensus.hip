// silo_gpu_consensus.hip — K15, the consensus call behind Consensus / AminoAcidConsensus: for count tables as a
// Mutations scan leaves them — counts[table][position][valid symbol] — one character per (table, position) and four sums per
// table (ambiguous, low coverage, deleted, differences from the reference).  Takes no store.
//
// Kernel:
//   k_consensus_call<N>   a block per 256 positions of one table (grid.y = table): the block's slab of the table through LDS with
//                         16-byte loads, then a thread per position: depth, need, selection steps in registers, the character,
//                         four ballots per wave, one integer add per block and sum (silo_gpu_consensus_call)
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t CONSENSUS_THREADS = SILO_GPU_CONSENSUS_THREADS;
constexpr uint32_t CONSENSUS_WAVES = CONSENSUS_THREADS / 64u;
constexpr uint32_t NUC_VALID = 5;   // "-ACGT"
constexpr uint32_t AA_VALID = 22;   // "-ACDEFGHIKLMNPQRSTVWY*"

/// The character of a set of nucleotides, bit k of `acgt` = the k-th of ACGT: the symbol itself or its IUPAC code.  Sixteen bytes
/// in two registers, indexed by shifts.
__device__ __forceinline__ char iupacOf(uint32_t acgt) {
   constexpr uint64_t LOW = 0x565352474D43413FULL;   // sets 0 .. 7, from the low byte:  ? A C M G R S V
   constexpr uint64_t HIGH = 0x4E42444B48595754ULL;  // sets 8 .. 15, from the low byte: T W Y H K D B N
   const uint64_t half = (acgt & 8u) != 0 ? HIGH : LOW;
   return static_cast<char>((half >> ((acgt & 7u) * 8u)) & 0xFFu);
}

__constant__ char AA_CALL_CHARS[AA_VALID + 1] = "-ACDEFGHIKLMNPQRSTVWY*";

/// grid = (ceil(n_positions / 256), n_tables); block (x, t) owns positions [256 x, 256 x + owned) of table t, thread i position
/// 256 x + i.  The owned * N words of the block are contiguous in the table; they start at any multiple of 4 bytes, so the block
/// loads the 16-byte quads that cover them — a quad that would reach outside the n_tables tables is loaded word by word, inside
/// only — into LDS, where a thread finds its N words at a stride of N (5: no bank conflict; 22: two lanes a bank).
/// Per position: depth = sum of the counts; below min_depth the missing symbol.  Otherwise need = ceil(depth * threshold) as K4
/// computes its bound (IEEE double product, ceil, then integers), and selection steps over the N counts in registers: a step
/// takes the highest count below the last one taken and adds every symbol that has it; the steps end when the sum reaches need
/// (it reaches depth >= need once every count above 0 is taken).  `cut` is the last count taken: the call's symbols are those
/// with count >= cut, ties included whatever their order.  Every loop runs over N, a template constant; `c` is indexed by
/// unrolled constants only (no scratch).  Nothing read from the table is used as an index.
/// The four sums: a ballot per wave and flag, the waves' counts through LDS, then threads 0 .. 3 add the block's sum to the
/// table's word — integer adds into words this call has cleared on the same stream: the same on every run.
template <uint32_t N>
__global__ __launch_bounds__(CONSENSUS_THREADS) void k_consensus_call(
   const uint32_t* __restrict__ counts, uint32_t n_positions, const uint8_t* __restrict__ reference_index, double threshold, uint32_t min_depth,
   char* __restrict__ out_chars, uint32_t* __restrict__ out_summary
) {
   __shared__ __attribute__((aligned(16))) uint32_t s_slab[CONSENSUS_THREADS * N + 4u];
   __shared__ uint32_t s_flags[CONSENSUS_WAVES][4];
   const uint32_t table = blockIdx.y;
   const uint32_t first = blockIdx.x * CONSENSUS_THREADS;
   const uint32_t owned = min(CONSENSUS_THREADS, n_positions - first);
   const size_t table_words = static_cast<size_t>(n_positions) * N;
   const auto all_words = static_cast<int64_t>(table_words * gridDim.y);
   const auto slab_begin = static_cast<int64_t>(table * table_words + static_cast<size_t>(first) * N);  // word of counts
   const uint32_t* slab = counts + slab_begin;
   const auto lead = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(slab) >> 2) & 3u);  // words from the 16-byte boundary below
   const uint32_t* aligned = slab - lead;
   const uint32_t quads = (lead + owned * N + 3u) / 4u;
   for (uint32_t quad = threadIdx.x; quad < quads; quad += CONSENSUS_THREADS) {
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

   bool ambiguous = false, low = false, deleted = false, differs = false;
   if (threadIdx.x < owned) {
      const uint32_t position = first + threadIdx.x;
      uint32_t c[N];
      uint32_t depth = 0;
#pragma unroll
      for (uint32_t s = 0; s < N; ++s) {
         c[s] = s_slab[lead + threadIdx.x * N + s];
         depth += c[s];
      }
      char call = N == NUC_VALID ? 'N' : 'X';
      low = depth < min_depth;
      if (!low) {
         const auto need = static_cast<uint32_t>(ceil(static_cast<double>(depth) * threshold));
         uint32_t cut = 0;
#pragma unroll
         for (uint32_t s = 0; s < N; ++s) {
            cut = max(cut, c[s]);
         }
         uint32_t sum = 0;
#pragma unroll
         for (uint32_t s = 0; s < N; ++s) {
            sum += c[s] == cut ? c[s] : 0u;
         }
         for (uint32_t step = 1; step < N; ++step) {  // (rolled: nothing in a step is indexed by it)
            if (sum >= need) {
               break;
            }
            uint32_t next = 0;
#pragma unroll
            for (uint32_t s = 0; s < N; ++s) {
               next = max(next, c[s] < cut ? c[s] : 0u);
            }
#pragma unroll
            for (uint32_t s = 0; s < N; ++s) {
               sum += c[s] == next ? c[s] : 0u;
            }
            cut = next;
         }
         uint32_t taken = 0;  // bit s: symbol s is in the call (cut > 0: depth >= 1 and the steps end on a count above 0)
#pragma unroll
         for (uint32_t s = 0; s < N; ++s) {
            taken |= (c[s] >= cut ? 1u : 0u) << s;
         }
         ambiguous = (taken & (taken - 1u)) != 0;
         if (N == NUC_VALID) {
            call = (taken & 1u) != 0 ? (ambiguous ? 'N' : '-') : iupacOf(taken >> 1);
         } else if (!ambiguous) {
            call = AA_CALL_CHARS[__ffs(static_cast<int>(taken)) - 1];
         }
         deleted = taken == 1u;
         differs = !ambiguous && static_cast<uint32_t>(__ffs(static_cast<int>(taken)) - 1) != reference_index[position];
      }
      out_chars[static_cast<size_t>(table) * n_positions + position] = call;
   }

   const uint32_t wave = threadIdx.x / 64u;
   const auto ambiguous_lanes = static_cast<uint32_t>(__popcll(__ballot(ambiguous)));
   const auto low_lanes = static_cast<uint32_t>(__popcll(__ballot(low)));
   const auto deleted_lanes = static_cast<uint32_t>(__popcll(__ballot(deleted)));
   const auto differing_lanes = static_cast<uint32_t>(__popcll(__ballot(differs)));
   if ((threadIdx.x & 63u) == 0) {
      s_flags[wave][0] = ambiguous_lanes;
      s_flags[wave][1] = low_lanes;
      s_flags[wave][2] = deleted_lanes;
      s_flags[wave][3] = differing_lanes;
   }
   __syncthreads();
   if (threadIdx.x < 4) {
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t w = 0; w < CONSENSUS_WAVES; ++w) {
         sum += s_flags[w][threadIdx.x];
      }
      if (sum != 0) {
         atomicAdd(out_summary + static_cast<size_t>(table) * 4u + threadIdx.x, sum);
      }
   }
}

}  // namespace

extern "C" {

int silo_gpu_consensus_call(
   int alphabet, const uint32_t* counts_dev, uint32_t n_tables, uint32_t n_positions, const uint8_t* reference_index_dev, double threshold,
   uint32_t min_depth, char* out_chars_dev, uint32_t* out_summary_dev, void* stream
) {
   if (alphabet != SILO_GPU_ALPHABET_NUCLEOTIDE && alphabet != SILO_GPU_ALPHABET_AMINO_ACID) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_consensus_call: unknown alphabet");
   }
   if (counts_dev == nullptr || reference_index_dev == nullptr || out_chars_dev == nullptr || out_summary_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_consensus_call: a buffer is NULL");
   }
   if (!(threshold > 0.0 && threshold <= 1.0)) {  // (NaN fails both)
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_consensus_call: the threshold is not in (0, 1]");
   }
   if (min_depth == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_consensus_call: min_depth is 0");
   }
   if (n_tables > SILO_GPU_MAX_CONSENSUS_TABLES) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_consensus_call: more tables than SILO_GPU_MAX_CONSENSUS_TABLES");
   }
   if ((reinterpret_cast<uintptr_t>(counts_dev) & 3u) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_consensus_call: the count tables are not 4-byte aligned");
   }
   if (n_tables == 0 || n_positions == 0) {
      return SILO_GPU_OK;
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   HIP_TRY(hipMemsetAsync(out_summary_dev, 0, static_cast<size_t>(n_tables) * 4u * sizeof(uint32_t), hip_stream));
   const dim3 grid((n_positions + CONSENSUS_THREADS - 1u) / CONSENSUS_THREADS, n_tables);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_consensus_call<NUC_VALID><<<grid, CONSENSUS_THREADS, 0, hip_stream>>>(
         counts_dev, n_positions, reference_index_dev, threshold, min_depth, out_chars_dev, out_summary_dev
      );
   } else {
      k_consensus_call<AA_VALID><<<grid, CONSENSUS_THREADS, 0, hip_stream>>>(
         counts_dev, n_positions, reference_index_dev, threshold, min_depth, out_chars_dev, out_summary_dev
      );
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
