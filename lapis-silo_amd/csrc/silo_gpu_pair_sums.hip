// silo_gpu_pair_sums.hip — K24, the pairwise sums of count tables behind MeanDistances / AminoAcidMeanDistances: for
// 1 .. 64 count tables as a Mutations scan leaves them — counts[table][position][valid symbol] — and up to 256 ranges of positions,
// per range and pair of tables g <= h the 128-bit sums of the differing and of the compared pairs of rows and the number of
// segregating sites (g == h) or fixed differences (g < h).  An integer GEMM, D = sum_p C_p C_p^T with C_p of G x N.  Takes no store.
//
// Kernel:
//   k_table_pair_sums<N>   a block per job = (range, chunk of 128 positions of it, 16 x 16 tile of pairs in the upper triangle), a
//                          thread per pair; 16 positions at a time the slabs of the tile's 16 + 16 tables through LDS with 16-byte
//                          loads, their coverages summed once; the 128-bit sums and the sites counter in registers over the chunk;
//                          at most five 64-bit integer atomics per thread, and one more per sum whose low word wrapped
//                          (silo_gpu_table_pair_sums)
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t THREADS = 256;
constexpr uint32_t TILE = SILO_GPU_PAIR_SUM_TILE;                     // tables of a side of a tile of pairs
constexpr uint32_t POSITION_TILE = SILO_GPU_PAIR_SUM_POSITION_TILE;   // positions staged at a time
constexpr uint32_t CHUNK = SILO_GPU_PAIR_SUM_CHUNK;                   // positions of a range that a block owns
constexpr uint32_t WORDS = SILO_GPU_PAIR_SUM_WORDS;
constexpr uint32_t MAX_RANGES = SILO_GPU_MAX_PAIR_SUM_RANGES;
constexpr uint32_t NUC_VALID = 5;   // "-ACGT"
constexpr uint32_t AA_VALID = 22;   // "-ACDEFGHIKLMNPQRSTVWY*"
constexpr uint32_t COVERAGE_STRIDE = POSITION_TILE + 1u;  // odd: the 16 tables of a side lie on 16 banks
static_assert(THREADS == TILE * TILE && CHUNK % POSITION_TILE == 0);

/// The ranges and where the chunks of each begin among the chunks of all, passed by value (3 KiB of kernel arguments): no upload,
/// nothing to keep alive.  Read with indices that are the same for a whole block.
struct PairSumRanges {
   uint32_t first[MAX_RANGES];
   uint32_t end[MAX_RANGES];
   uint32_t chunk_begin[MAX_RANGES + 1u];  // chunk_begin[n_ranges] = the chunks of all ranges
};

/// Words between the slabs of two tables in LDS: odd, so that the 16 tables a half-wave reads at one (position, symbol) lie on 16
/// different banks (a 4-byte LDS read takes its bank from the word address modulo 32).
template <uint32_t N>
constexpr uint32_t slabStride() {
   return (POSITION_TILE * N) | 1u;
}

__device__ inline void add128(uint64_t& lo, uint64_t& hi, uint64_t term) {
   lo += term;
   hi += lo < term ? 1u : 0u;
}

/// Adds a block's 128-bit partial sum to the two words at `at`: the carry of the low word's add goes with the high word.
__device__ inline void atomicAdd128(unsigned long long* at, uint64_t lo, uint64_t hi) {
   if (lo != 0) {
      const unsigned long long before = atomicAdd(at, static_cast<unsigned long long>(lo));
      hi += before + lo < before ? 1u : 0u;
   }
   if (hi != 0) {
      atomicAdd(at + 1, static_cast<unsigned long long>(hi));
   }
}

/// grid = (the chunks of all ranges) x (the tiles of pairs with tile_g <= tile_h), the tile the fastest.  Thread t of a block is the
/// pair g = 16 tile_g + t / 16, h = 16 tile_h + t % 16; it works iff g <= h < n_tables, but every thread stages and meets the barriers.
/// Per 16 positions: the `owned * N` words of a table's slab are contiguous in `counts`; they start at any multiple of 4 bytes, so
/// 16 threads per table load the 16-byte quads that cover them — a quad that would reach outside the n_tables tables is loaded word by
/// word, inside only — and write the words of the slab into LDS (4-byte stores: the stride is odd); a tile on the diagonal stages
/// its tables once.  Then a thread per (table, position) sums the coverage.  Then a thread walks the positions: the g row's words are
/// the same for the 16 lanes of a row (a broadcast), the h rows' words lie on 16 banks.  Nothing read from a table is used as an index.
template <uint32_t N>
__global__ __launch_bounds__(THREADS) void k_table_pair_sums(
   const uint32_t* __restrict__ counts, uint32_t n_tables, uint32_t n_positions, const PairSumRanges ranges, uint32_t n_ranges, uint32_t n_tiles,
   unsigned long long* __restrict__ out
) {
   constexpr uint32_t STRIDE = slabStride<N>();
   __shared__ uint32_t s_slab[2][TILE * STRIDE];
   __shared__ uint32_t s_coverage[2][TILE * COVERAGE_STRIDE];

   // the job: which range, which chunk of it, which tile of pairs
   const uint32_t tile = blockIdx.x % n_tiles;
   const uint32_t chunk = blockIdx.x / n_tiles;
   uint32_t range = 0;  // the last range whose chunks begin at or before `chunk` (every range has a chunk)
   for (uint32_t above = n_ranges; above - range > 1;) {
      const uint32_t middle = (range + above) / 2u;
      if (ranges.chunk_begin[middle] <= chunk) {
         range = middle;
      } else {
         above = middle;
      }
   }
   const uint32_t tiles_per_side = (n_tables + TILE - 1u) / TILE;
   uint32_t tile_g = 0;
   uint32_t tile_h = tile;
   while (tile_h >= tiles_per_side - tile_g) {  // row tile_g of the triangle holds tiles_per_side - tile_g tiles
      tile_h -= tiles_per_side - tile_g;
      ++tile_g;
   }
   tile_h += tile_g;
   const bool diagonal = tile_g == tile_h;
   const uint32_t sides = diagonal ? 1u : 2u;
   const uint32_t chunk_first = ranges.first[range] + (chunk - ranges.chunk_begin[range]) * CHUNK;
   const uint32_t chunk_positions = min(CHUNK, ranges.end[range] - chunk_first);

   const uint32_t row = threadIdx.x / TILE;
   const uint32_t column = threadIdx.x % TILE;
   const uint32_t g = tile_g * TILE + row;
   const uint32_t h = tile_h * TILE + column;
   const bool works = g <= h && h < n_tables;
   const bool same = g == h;
   const size_t table_words = static_cast<size_t>(n_positions) * N;
   const auto all_words = static_cast<int64_t>(table_words * n_tables);
   const uint32_t* slab_g = s_slab[0] + row * STRIDE;
   const uint32_t* slab_h = s_slab[diagonal ? 0 : 1] + column * STRIDE;
   const uint32_t* coverage_g = s_coverage[0] + row * COVERAGE_STRIDE;
   const uint32_t* coverage_h = s_coverage[diagonal ? 0 : 1] + column * COVERAGE_STRIDE;

   uint64_t diff_lo = 0, diff_hi = 0, cmp_lo = 0, cmp_hi = 0;
   uint32_t sites = 0;
   for (uint32_t done = 0; done < chunk_positions; done += POSITION_TILE) {
      const uint32_t first = chunk_first + done;
      const uint32_t owned = min(POSITION_TILE, chunk_positions - done);
      for (uint32_t side = 0; side < sides; ++side) {
         const uint32_t table = (side == 0 ? tile_g : tile_h) * TILE + row;  // 16 threads per table
         if (table < n_tables) {
            const auto slab_begin = static_cast<int64_t>(table * table_words + static_cast<size_t>(first) * N);  // word of counts
            const uint32_t* slab = counts + slab_begin;
            const auto lead = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(slab) >> 2) & 3u);  // words from the 16-byte boundary below
            const uint32_t* aligned = slab - lead;
            const uint32_t slab_words = owned * N;
            const uint32_t quads = (lead + slab_words + 3u) / 4u;
            uint32_t* to = s_slab[side] + row * STRIDE;
            for (uint32_t quad = column; quad < quads; quad += TILE) {
               const int64_t word = slab_begin - lead + static_cast<int64_t>(quad) * 4;  // of counts; below 0 or past the end: not ours to read
               uint32_t loaded[4] = {0, 0, 0, 0};
               if (word >= 0 && word + 4 <= all_words) {
                  const uint4 four = *reinterpret_cast<const uint4*>(aligned + quad * 4u);
                  loaded[0] = four.x;
                  loaded[1] = four.y;
                  loaded[2] = four.z;
                  loaded[3] = four.w;
               } else {
#pragma unroll
                  for (uint32_t k = 0; k < 4; ++k) {
                     if (word + k >= 0 && word + k < all_words) {
                        loaded[k] = aligned[quad * 4u + k];
                     }
                  }
               }
#pragma unroll
               for (uint32_t k = 0; k < 4; ++k) {
                  const uint32_t at = quad * 4u + k - lead;  // of the slab; wraps below 0: not a word of it
                  if (at < slab_words) {
                     to[at] = loaded[k];
                  }
               }
            }
         }
      }
      __syncthreads();
      for (uint32_t entry = threadIdx.x; entry < sides * TILE * POSITION_TILE; entry += THREADS) {
         const uint32_t side = entry / (TILE * POSITION_TILE);
         const uint32_t of_side = (entry % (TILE * POSITION_TILE)) / POSITION_TILE;
         const uint32_t position = entry % POSITION_TILE;
         if ((side == 0 ? tile_g : tile_h) * TILE + of_side < n_tables && position < owned) {
            const uint32_t* cells = s_slab[side] + of_side * STRIDE + position * N;
            uint32_t coverage = 0;
#pragma unroll
            for (uint32_t s = 0; s < N; ++s) {
               coverage += cells[s];
            }
            s_coverage[side][of_side * COVERAGE_STRIDE + position] = coverage;
         }
      }
      __syncthreads();
      if (works) {
         for (uint32_t position = 0; position < owned; ++position) {
            const uint32_t* cells_g = slab_g + position * N;
            const uint32_t* cells_h = slab_h + position * N;
            uint64_t shared = 0;    // sum_s c_g c_h: at most cov_g cov_h
            uint32_t present = 0;   // symbols of g with a count above 0
#pragma unroll
            for (uint32_t s = 0; s < N; ++s) {
               const uint32_t of_g = cells_g[s];
               shared += static_cast<uint64_t>(of_g) * cells_h[s];
               present += of_g != 0 ? 1u : 0u;
            }
            const uint64_t covered_g = coverage_g[position];
            const uint64_t covered_h = coverage_h[position];
            const uint64_t product = covered_g * covered_h;
            if (same) {
               add128(diff_lo, diff_hi, (product - shared) / 2u);
               add128(cmp_lo, cmp_hi, covered_g == 0 ? 0u : covered_g * (covered_g - 1u) / 2u);  // below 2^64 before the halving
               sites += present >= 2 ? 1u : 0u;
            } else {
               add128(diff_lo, diff_hi, product - shared);
               add128(cmp_lo, cmp_hi, product);
               sites += product != 0 && shared == 0 ? 1u : 0u;
            }
         }
      }
      __syncthreads();  // the slabs are read: the next positions may overwrite them
   }
   if (!works) {
      return;
   }
   const size_t pairs = static_cast<size_t>(n_tables) * (n_tables + 1u) / 2u;
   const size_t pair = static_cast<size_t>(g) * n_tables - static_cast<size_t>(g) * (g + 1u) / 2u + h;  // the rows before g hold n_tables - i pairs each
   unsigned long long* record = out + (static_cast<size_t>(range) * pairs + pair) * WORDS;
   atomicAdd128(record, diff_lo, diff_hi);
   atomicAdd128(record + 2, cmp_lo, cmp_hi);
   if (sites != 0) {
      atomicAdd(record + 4, static_cast<unsigned long long>(sites));
   }
}

}  // namespace

extern "C" {

int silo_gpu_table_pair_sums(
   int alphabet, const uint32_t* counts_dev, uint32_t n_tables, uint32_t n_positions, const uint32_t* ranges, uint32_t n_ranges, uint64_t* out_dev,
   void* stream
) {
   if (alphabet != SILO_GPU_ALPHABET_NUCLEOTIDE && alphabet != SILO_GPU_ALPHABET_AMINO_ACID) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: unknown alphabet");
   }
   if (counts_dev == nullptr || ranges == nullptr || out_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: a buffer is NULL");
   }
   if (n_tables == 0 || n_tables > SILO_GPU_MAX_PAIR_SUM_TABLES) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: the number of tables is not in [1, SILO_GPU_MAX_PAIR_SUM_TABLES]");
   }
   if (n_ranges == 0 || n_ranges > MAX_RANGES) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: the number of ranges is not in [1, SILO_GPU_MAX_PAIR_SUM_RANGES]");
   }
   if (n_positions == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: tables without positions hold no range");
   }
   if ((reinterpret_cast<uintptr_t>(counts_dev) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_dev) & 7u) != 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: the count tables are not 4-byte or the records not 8-byte aligned");
   }
   PairSumRanges range_args{};
   uint64_t chunks = 0;
   for (uint32_t r = 0; r < n_ranges; ++r) {
      const uint32_t first = ranges[2u * r];
      const uint32_t end = ranges[2u * r + 1u];
      if (first >= end || end > n_positions) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: a range is empty or ends past the positions of the tables");
      }
      range_args.first[r] = first;
      range_args.end[r] = end;
      range_args.chunk_begin[r] = static_cast<uint32_t>(chunks);
      chunks += (static_cast<uint64_t>(end - first) + CHUNK - 1u) / CHUNK;  // at most 2^25 a range: the sum of 256 fits 2^33
      if (chunks > INT32_MAX) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: more jobs than a grid holds");
      }
   }
   for (uint32_t r = n_ranges; r <= MAX_RANGES; ++r) {
      range_args.chunk_begin[r] = static_cast<uint32_t>(chunks);
   }
   const uint32_t tiles_per_side = (n_tables + TILE - 1u) / TILE;
   const uint32_t n_tiles = tiles_per_side * (tiles_per_side + 1u) / 2u;
   const uint64_t blocks = chunks * n_tiles;
   if (blocks > INT32_MAX) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_table_pair_sums: more jobs than a grid holds");
   }
   const size_t records = static_cast<size_t>(n_ranges) * (static_cast<size_t>(n_tables) * (n_tables + 1u) / 2u);
   auto hip_stream = static_cast<hipStream_t>(stream);
   HIP_TRY(hipMemsetAsync(out_dev, 0, records * WORDS * sizeof(uint64_t), hip_stream));
   auto* out = reinterpret_cast<unsigned long long*>(out_dev);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_table_pair_sums<NUC_VALID><<<static_cast<uint32_t>(blocks), THREADS, 0, hip_stream>>>(counts_dev, n_tables, n_positions, range_args, n_ranges, n_tiles, out);
   } else {
      k_table_pair_sums<AA_VALID><<<static_cast<uint32_t>(blocks), THREADS, 0, hip_stream>>>(counts_dev, n_tables, n_positions, range_args, n_ranges, n_tiles, out);
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
