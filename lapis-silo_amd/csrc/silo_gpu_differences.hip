// silo_gpu_differences.hip — K18, each row's differences from the reference behind MutationsPerSequence /
// AminoAcidMutationsPerSequence: for n rows of characters as silo_gpu_reconstruct_sequences yields them for every
// layout, per row the ordered list of its substitutions, ambiguous cells and the starts and closes of its runs of deletions and of
// the missing symbol, as one compact list of words over all rows, with the offsets of the rows in it and four cell counts per row.
// Takes no store.
//
// Kernels:
//   k_difference_count    a block per (chunk of DIFFERENCE_CHUNK bytes of a row, row), a thread per aligned 16 bytes: the class of
//                         every cell, the flags of the cells that emit a word; the block's words and its four cell counts
//   k_difference_rows     a wave per row: the row's chunk counts become starts within the row, its cell counts are summed
//   k_difference_offsets  one block: the rows' totals become the offsets
//   k_difference_write    the blocks of the count pass again: the flags recomputed, each word at its chunk's start plus its rank
// Nowhere does a block wait for another, nothing is added into memory: what blocks hand on is one plain store per value each.
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t DIFFERENCE_THREADS = 256;
constexpr uint32_t DIFFERENCE_WAVES = DIFFERENCE_THREADS / 64u;
constexpr uint32_t QUAD_BYTES = 16;                               // what a thread reads: one aligned uint4
constexpr uint32_t DIFFERENCE_CHUNK = SILO_GPU_DIFFERENCE_CHUNK;  // bytes of a row per block
constexpr uint32_t STATS = SILO_GPU_DIFFERENCE_STATS;
constexpr uint32_t OFFSET_THREADS = 1024;
static_assert(DIFFERENCE_CHUNK == DIFFERENCE_THREADS * QUAD_BYTES);
static_assert((SILO_GPU_MAX_DIFFERENCE_POSITIONS - 1u) <= (UINT32_MAX >> 9), "a position fits above the 9 low bits of a record word");

/// The class of a cell; OUTSIDE is what a byte of a thread's 16 has that is no cell of the row, and what lies left of cell 0.
enum CellClass : uint32_t { SAME = 0, SUBSTITUTION = 1, DELETION = 2, MISSING = 3, AMBIGUOUS = 4, OUTSIDE = 5 };

/// Bit (c & 63) for every character c of `symbols` in [64 * half, 64 * half + 64): the valid mutation symbols are all below 128.
constexpr uint64_t validBits(const char* symbols, uint32_t half) {
   uint64_t bits = 0;
   for (const char* symbol = symbols; *symbol != '\0'; ++symbol) {
      const auto c = static_cast<uint32_t>(static_cast<uint8_t>(*symbol));
      if (c / 64u == half) {
         bits |= uint64_t{1} << (c & 63u);
      }
   }
   return bits;
}

/// The valid mutation symbols in the order of Nucleotide / AminoAcid::VALID_MUTATION_SYMBOLS (host/symbols.h), as K10 lists them.
struct NucleotideCells {
   static constexpr uint32_t MISSING_SYMBOL = 'N';
   static constexpr uint64_t VALID_LOW = validBits("-ACGT", 0);
   static constexpr uint64_t VALID_HIGH = validBits("-ACGT", 1);
};
struct AminoAcidCells {
   static constexpr uint32_t MISSING_SYMBOL = 'X';
   static constexpr uint64_t VALID_LOW = validBits("-ACDEFGHIKLMNPQRSTVWY*", 0);
   static constexpr uint64_t VALID_HIGH = validBits("-ACDEFGHIKLMNPQRSTVWY*", 1);
};

template <typename Alphabet>
__device__ __forceinline__ uint32_t classOf(uint32_t c, uint32_t reference) {
   if (c == Alphabet::MISSING_SYMBOL) {
      return MISSING;
   }
   const uint64_t bits = c < 64u ? Alphabet::VALID_LOW : Alphabet::VALID_HIGH;
   if (c >= 128u || ((bits >> (c & 63u)) & 1u) == 0) {
      return AMBIGUOUS;
   }
   if (c == reference) {
      return SAME;
   }
   return c == '-' ? DELETION : SUBSTITUTION;
}

__device__ __forceinline__ bool isRun(uint32_t cell_class) {
   return cell_class == DELETION || cell_class == MISSING;
}

/// What a thread knows of its 16 bytes: bit j of a mask is byte j, which is the cell at position first + j where it is one.
struct QuadCells {
   int64_t first;        // position of byte 0: below 0 in a row's first quad, where the row does not start on a 16-byte boundary
   uint32_t bytes[4];    // the characters (0 where the byte is no cell of the row)
   uint32_t emits;       // the cell writes a record word
   uint32_t closes;      // ... and that word is a close
   uint32_t of_class[STATS];  // the cell is a substitution / deleted / missing / ambiguous
};

/// The quad `quad` (counted from the 16-byte boundary at or below the row's first byte) of row `row`, for every thread of a wave
/// at once (it shuffles): thread i of the wave must hold quad q + i, so that the lane before holds the cells to the left.
/// The quad is loaded as one uint4 where all 16 bytes lie inside the n_rows * positions characters (they may belong to the rows
/// before and after: those bytes are masked, not cells) and byte by byte, inside only, where it would reach outside — as
/// k_mutations_compare loads a quad at the ends of its tables.  The 16 reference characters start at any alignment: one 16-byte
/// copy where all are positions of the sequence, byte by byte otherwise.  Left of a thread's first cell: the class of the last
/// byte of the lane before; the first lane of a wave reads the ONE byte at position first - 1 of the same row (and the
/// reference's) where first > 0.  Left of position 0 is OUTSIDE, whatever row r - 1 ends with.
template <typename Alphabet>
__device__ __forceinline__ QuadCells classifyQuad(
   const uint8_t* __restrict__ chars, const uint8_t* __restrict__ reference, int64_t row_begin, int64_t all_bytes, int64_t positions, int64_t first
) {
   QuadCells cells;
   cells.first = first;
   uint32_t theirs[4] = {0, 0, 0, 0};
#pragma unroll
   for (uint32_t k = 0; k < 4; ++k) {
      cells.bytes[k] = 0;
   }
   const bool holds_cells = first < positions;  // (first > -16 always)
   if (holds_cells) {
      const int64_t begin = row_begin + first;  // byte of chars; a multiple of 16 bytes from the boundary: aligned
      if (begin >= 0 && begin + QUAD_BYTES <= all_bytes) {
         const uint4 quad = *reinterpret_cast<const uint4*>(chars + begin);
         cells.bytes[0] = quad.x;
         cells.bytes[1] = quad.y;
         cells.bytes[2] = quad.z;
         cells.bytes[3] = quad.w;
      } else {
#pragma unroll
         for (uint32_t j = 0; j < QUAD_BYTES; ++j) {
            if (begin + j >= 0 && begin + j < all_bytes) {
               cells.bytes[j / 4u] |= static_cast<uint32_t>(chars[begin + j]) << (8u * (j % 4u));
            }
         }
      }
      if (first >= 0 && first + QUAD_BYTES <= positions) {
         __builtin_memcpy(theirs, reference + first, QUAD_BYTES);
      } else {
#pragma unroll
         for (uint32_t j = 0; j < QUAD_BYTES; ++j) {
            if (first + j >= 0 && first + j < positions) {
               theirs[j / 4u] |= static_cast<uint32_t>(reference[first + j]) << (8u * (j % 4u));
            }
         }
      }
   }
   uint32_t classes[QUAD_BYTES];  // indexed by unrolled constants only
#pragma unroll
   for (uint32_t j = 0; j < QUAD_BYTES; ++j) {
      const bool is_cell = first + j >= 0 && first + j < positions;
      const uint32_t c = (cells.bytes[j / 4u] >> (8u * (j % 4u))) & 0xFFu;
      const uint32_t r = (theirs[j / 4u] >> (8u * (j % 4u))) & 0xFFu;
      classes[j] = is_cell ? classOf<Alphabet>(c, r) : static_cast<uint32_t>(OUTSIDE);
      if (!is_cell) {
         cells.bytes[j / 4u] &= ~(0xFFu << (8u * (j % 4u)));
      }
   }
   uint32_t left = __shfl_up(classes[QUAD_BYTES - 1u], 1);
   if ((threadIdx.x & 63u) == 0) {
      left = OUTSIDE;
      if (first > 0 && holds_cells) {
         left = classOf<Alphabet>(chars[row_begin + first - 1], reference[first - 1]);
      }
   }
   cells.emits = 0;
   cells.closes = 0;
#pragma unroll
   for (uint32_t k = 0; k < STATS; ++k) {
      cells.of_class[k] = 0;
   }
#pragma unroll
   for (uint32_t j = 0; j < QUAD_BYTES; ++j) {
      const uint32_t mine = classes[j];
      const bool close = mine == SAME && isRun(left);
      const bool emit = mine == SUBSTITUTION || mine == AMBIGUOUS || (isRun(mine) && left != mine) || close;
      cells.emits |= (emit ? 1u : 0u) << j;
      cells.closes |= (close ? 1u : 0u) << j;
      cells.of_class[0] |= (mine == SUBSTITUTION ? 1u : 0u) << j;
      cells.of_class[1] |= (mine == DELETION ? 1u : 0u) << j;
      cells.of_class[2] |= (mine == MISSING ? 1u : 0u) << j;
      cells.of_class[3] |= (mine == AMBIGUOUS ? 1u : 0u) << j;
      left = mine;
   }
   return cells;
}

/// The position of byte 0 of thread threadIdx.x's quad in block (chunk, row) of the two passes over the characters.
__device__ __forceinline__ int64_t firstPositionOfThread(const uint8_t* chars, int64_t row_begin) {
   const auto lead = static_cast<int64_t>(reinterpret_cast<uintptr_t>(chars + row_begin) & (QUAD_BYTES - 1u));  // bytes from the boundary below
   return (static_cast<int64_t>(blockIdx.x) * DIFFERENCE_THREADS + threadIdx.x) * QUAD_BYTES - lead;
}

template <typename T>
__device__ __forceinline__ T waveSum(T value) {
#pragma unroll
   for (uint32_t distance = 32; distance != 0; distance /= 2u) {
      value += __shfl_xor(value, static_cast<int>(distance));
   }
   return value;
}

/// The sum over the lanes up to and including this one.
__device__ __forceinline__ uint32_t waveInclusiveSum(uint32_t value) {
   const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
   for (uint32_t distance = 1; distance < 64u; distance *= 2u) {
      const uint32_t below = __shfl_up(value, distance);
      if (lane >= distance) {
         value += below;
      }
   }
   return value;
}

/// grid = (chunks, n_rows).  counts[row * chunks + chunk] = the words of the block's cells; partials[(row * chunks + chunk) * 4 + k]
/// = its cells of class k.  A block holds at most DIFFERENCE_CHUNK cells, so the four cell counts travel as 16-bit fields of one
/// 64-bit sum.  Every block writes its five words, a chunk without cells (a row that starts on a boundary has one fewer) zeros.
template <typename Alphabet>
__global__ __launch_bounds__(DIFFERENCE_THREADS) void k_difference_count(
   const uint8_t* __restrict__ chars, const uint8_t* __restrict__ reference, uint32_t positions, int64_t all_bytes, uint32_t* __restrict__ counts,
   uint32_t* __restrict__ partials
) {
   static_assert(DIFFERENCE_CHUNK < (1u << 16));
   __shared__ uint32_t s_words[DIFFERENCE_WAVES];
   __shared__ uint64_t s_cells[DIFFERENCE_WAVES];
   const int64_t row_begin = static_cast<int64_t>(blockIdx.y) * positions;
   const QuadCells cells = classifyQuad<Alphabet>(chars, reference, row_begin, all_bytes, positions, firstPositionOfThread(chars, row_begin));
   uint64_t of_class = 0;
#pragma unroll
   for (uint32_t k = 0; k < STATS; ++k) {
      of_class |= static_cast<uint64_t>(__popc(cells.of_class[k])) << (16u * k);
   }
   const uint32_t words = waveSum(static_cast<uint32_t>(__popc(cells.emits)));
   of_class = waveSum(of_class);
   if ((threadIdx.x & 63u) == 0) {
      s_words[threadIdx.x / 64u] = words;
      s_cells[threadIdx.x / 64u] = of_class;
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t block_words = 0;
      uint64_t block_cells = 0;
#pragma unroll
      for (uint32_t wave = 0; wave < DIFFERENCE_WAVES; ++wave) {
         block_words += s_words[wave];
         block_cells += s_cells[wave];
      }
      const size_t block = static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
      counts[block] = block_words;
#pragma unroll
      for (uint32_t k = 0; k < STATS; ++k) {
         partials[block * STATS + k] = static_cast<uint32_t>(block_cells >> (16u * k)) & 0xFFFFu;
      }
   }
}

/// grid = ceil(n_rows / DIFFERENCE_WAVES), a wave per row, 64 chunks at a time: counts[row * chunks + chunk] becomes the words of
/// the row's chunks before it, offsets[row + 1] the row's words (k_difference_offsets sums them up), stats[row * 4 + k] the sum
/// of its partials.
__global__ __launch_bounds__(DIFFERENCE_THREADS) void k_difference_rows(
   uint32_t n_rows, uint32_t chunks, uint32_t* __restrict__ counts, const uint32_t* __restrict__ partials, uint32_t* __restrict__ offsets,
   uint32_t* __restrict__ stats
) {
   const uint32_t row = blockIdx.x * DIFFERENCE_WAVES + threadIdx.x / 64u;  // the same for the whole wave
   if (row >= n_rows) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const size_t row_blocks = static_cast<size_t>(row) * chunks;
   uint32_t before = 0;
   uint32_t of_class[STATS] = {0, 0, 0, 0};
   for (uint32_t base = 0; base < chunks; base += 64u) {
      const uint32_t chunk = base + lane;
      uint32_t words = 0;
      if (chunk < chunks) {
         words = counts[row_blocks + chunk];
#pragma unroll
         for (uint32_t k = 0; k < STATS; ++k) {
            of_class[k] += partials[(row_blocks + chunk) * STATS + k];
         }
      }
      const uint32_t through = waveInclusiveSum(words);
      if (chunk < chunks) {
         counts[row_blocks + chunk] = before + through - words;
      }
      before += __shfl(through, 63);
   }
#pragma unroll
   for (uint32_t k = 0; k < STATS; ++k) {
      of_class[k] = waveSum(of_class[k]);
   }
   if (lane == 0) {
      offsets[row + 1u] = before;
#pragma unroll
      for (uint32_t k = 0; k < STATS; ++k) {
         stats[static_cast<size_t>(row) * STATS + k] = of_class[k];
      }
   }
}

/// One block.  offsets[1 .. n_rows] hold the rows' words and become their running sum; offsets[0] = 0.  A thread owns
/// ceil(n_rows / OFFSET_THREADS) consecutive rows (at most 10): their sum, the sums of the threads before it through a wave scan
/// and the waves' totals in LDS, then its rows again.
__global__ __launch_bounds__(OFFSET_THREADS) void k_difference_offsets(uint32_t n_rows, uint32_t* __restrict__ offsets) {
   __shared__ uint32_t s_waves[OFFSET_THREADS / 64u];
   const uint32_t per_thread = (n_rows + OFFSET_THREADS - 1u) / OFFSET_THREADS;
   const uint32_t begin = min(threadIdx.x * per_thread, n_rows);
   const uint32_t end = min(begin + per_thread, n_rows);
   uint32_t mine = 0;
   for (uint32_t row = begin; row < end; ++row) {
      mine += offsets[row + 1u];
   }
   const uint32_t through = waveInclusiveSum(mine);
   if ((threadIdx.x & 63u) == 63u) {
      s_waves[threadIdx.x / 64u] = through;
   }
   __syncthreads();
   uint32_t running = through - mine;
   for (uint32_t wave = 0; wave < threadIdx.x / 64u; ++wave) {
      running += s_waves[wave];
   }
   for (uint32_t row = begin; row < end; ++row) {
      running += offsets[row + 1u];
      offsets[row + 1u] = running;
   }
   if (threadIdx.x == 0) {
      offsets[0] = 0;
   }
}

/// grid = (chunks, n_rows), as k_difference_count.  The block's first word goes to offsets[row] + counts[row * chunks + chunk] (the
/// start within the row, from k_difference_rows); a thread's first word comes after those of the waves before it (LDS) and of the
/// lanes before it (a scan over the wave: a thread holds up to 16 words, so a ballot's popcount does not rank them), its further
/// words follow in position order.  Every index — it derives from counts in memory — is compared with `capacity` before the store;
/// a block whose first word lies at or past it stores nothing.
template <typename Alphabet>
__global__ __launch_bounds__(DIFFERENCE_THREADS) void k_difference_write(
   const uint8_t* __restrict__ chars, const uint8_t* __restrict__ reference, uint32_t positions, int64_t all_bytes, const uint32_t* __restrict__ counts,
   const uint32_t* __restrict__ offsets, uint32_t capacity, uint32_t* __restrict__ records
) {
   __shared__ uint32_t s_words[DIFFERENCE_WAVES];
   const uint64_t start = static_cast<uint64_t>(offsets[blockIdx.y]) + counts[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x];
   if (start >= capacity) {  // the same for the whole block
      return;
   }
   const int64_t row_begin = static_cast<int64_t>(blockIdx.y) * positions;
   const QuadCells cells = classifyQuad<Alphabet>(chars, reference, row_begin, all_bytes, positions, firstPositionOfThread(chars, row_begin));
   const auto words = static_cast<uint32_t>(__popc(cells.emits));
   const uint32_t through = waveInclusiveSum(words);
   if ((threadIdx.x & 63u) == 63u) {
      s_words[threadIdx.x / 64u] = through;
   }
   __syncthreads();
   uint64_t at = start + through - words;
   for (uint32_t wave = 0; wave < threadIdx.x / 64u; ++wave) {
      at += s_words[wave];
   }
#pragma unroll
   for (uint32_t j = 0; j < QUAD_BYTES; ++j) {
      if (((cells.emits >> j) & 1u) != 0) {
         if (at < capacity) {
            const uint32_t byte = (cells.bytes[j / 4u] >> (8u * (j % 4u))) & 0xFFu;
            const auto position = static_cast<uint32_t>(cells.first + j);  // a cell: 0 <= position < positions
            records[at] = (position << 9u) | (((cells.closes >> j) & 1u) != 0 ? 0x100u : byte);
         }
         ++at;
      }
   }
}

template <typename Alphabet>
void launchPasses(
   const uint8_t* chars, uint32_t n_rows, uint32_t positions, const uint8_t* reference, uint32_t capacity, uint32_t* offsets, uint32_t* stats,
   uint32_t* records, uint32_t* scratch, hipStream_t stream
) {
   const uint32_t chunks = SILO_GPU_DIFFERENCE_CHUNKS(positions);
   const auto all_bytes = static_cast<int64_t>(n_rows) * positions;
   uint32_t* partials = scratch;  // [n_rows][chunks][STATS]
   uint32_t* counts = scratch + static_cast<size_t>(n_rows) * chunks * STATS;  // [n_rows][chunks]
   const dim3 grid(chunks, n_rows);
   k_difference_count<Alphabet><<<grid, DIFFERENCE_THREADS, 0, stream>>>(chars, reference, positions, all_bytes, counts, partials);
   k_difference_rows<<<(n_rows + DIFFERENCE_WAVES - 1u) / DIFFERENCE_WAVES, DIFFERENCE_THREADS, 0, stream>>>(n_rows, chunks, counts, partials, offsets, stats);
   k_difference_offsets<<<1, OFFSET_THREADS, 0, stream>>>(n_rows, offsets);
   if (capacity != 0) {
      k_difference_write<Alphabet><<<grid, DIFFERENCE_THREADS, 0, stream>>>(chars, reference, positions, all_bytes, counts, offsets, capacity, records);
   }
}

}  // namespace

extern "C" {

int silo_gpu_sequence_differences(
   int alphabet, const char* chars_dev, uint32_t n_rows, uint32_t positions, const char* reference_dev, uint32_t capacity, uint32_t* offsets_dev,
   uint32_t* stats_dev, uint32_t* records_dev, void* scratch_dev, void* stream
) {
   if (alphabet != SILO_GPU_ALPHABET_NUCLEOTIDE && alphabet != SILO_GPU_ALPHABET_AMINO_ACID) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sequence_differences: unknown alphabet");
   }
   if (chars_dev == nullptr || reference_dev == nullptr || offsets_dev == nullptr || stats_dev == nullptr || scratch_dev == nullptr ||
       (records_dev == nullptr && capacity != 0)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sequence_differences: a buffer is NULL");
   }
   if (((reinterpret_cast<uintptr_t>(offsets_dev) | reinterpret_cast<uintptr_t>(stats_dev) | reinterpret_cast<uintptr_t>(records_dev) |
         reinterpret_cast<uintptr_t>(scratch_dev)) &
        3u) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sequence_differences: the offsets, stats, records or scratch are not 4-byte aligned");
   }
   if (n_rows > SILO_GPU_MAX_DIFFERENCE_ROWS || positions > SILO_GPU_MAX_DIFFERENCE_POSITIONS) {
      return fail(
         SILO_GPU_ERR_INVALID_ARGUMENT,
         "silo_gpu_sequence_differences: more than SILO_GPU_MAX_DIFFERENCE_ROWS rows or more than SILO_GPU_MAX_DIFFERENCE_POSITIONS positions"
      );
   }
   if (static_cast<uint64_t>(n_rows) * positions >= (uint64_t{1} << 32)) {  // a list index, at most a word per cell, is a uint32
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_sequence_differences: n_rows * positions is 2^32 or more");
   }
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (n_rows == 0 || positions == 0) {
      HIP_TRY(hipMemsetAsync(offsets_dev, 0, (static_cast<size_t>(n_rows) + 1u) * sizeof(uint32_t), hip_stream));
      if (n_rows != 0) {
         HIP_TRY(hipMemsetAsync(stats_dev, 0, static_cast<size_t>(n_rows) * STATS * sizeof(uint32_t), hip_stream));
      }
      return SILO_GPU_OK;
   }
   const auto* chars = reinterpret_cast<const uint8_t*>(chars_dev);
   const auto* reference = reinterpret_cast<const uint8_t*>(reference_dev);
   auto* scratch = static_cast<uint32_t*>(scratch_dev);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      launchPasses<NucleotideCells>(chars, n_rows, positions, reference, capacity, offsets_dev, stats_dev, records_dev, scratch, hip_stream);
   } else {
      launchPasses<AminoAcidCells>(chars, n_rows, positions, reference, capacity, offsets_dev, stats_dev, records_dev, scratch, hip_stream);
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
