// silo_gpu_distance.hip — the pairwise distances behind DistanceMatrix (K10): for n rows of characters, per pair
// the positions where both rows hold a valid mutation symbol (compared) and where those two symbols differ (differing).
// Neither entry point takes a store: they start from the characters silo_gpu_reconstruct_sequences yields for every layout.
//
// Kernels:
//   k_distance_pack    one row of characters -> bit planes over positions (silo_gpu_distance_pack): a wave maps 64 consecutive
//                      characters through a 256-byte table, one ballot per plane is the plane's word
//   k_distance_pairs   an AND / XOR-popcount "GEMM" over the planes (silo_gpu_distance_pairs): a block owns a tile of
//                      DISTANCE_TILE x DISTANCE_TILE pairs on or above the diagonal, stages the words of its 2 x DISTANCE_TILE
//                      rows in LDS chunk by chunk, and WRITES each pair's two counts once
// and the same comparison as a yes / no per pair behind Clusters (K12):
//   k_distance_within  "differing <= max_distance and compared >= min_compared" as one BIT per pair (silo_gpu_distance_within): a
//                      block owns WITHIN_TILE_ROWS x WITHIN_TILE_COLS pairs at or right of the diagonal's word, four pairs per
//                      thread in registers, a wave's ballot is a finished word; it stops once no pair of its tile can be linked
//   k_adjacency_mirror the words left of the diagonal's word, transposed from the 64 x 64 bit blocks right of it
// and as a full matrix of weights behind MinimumSpanningTree (K13):
//   k_distance_weights the same tiles and the same walk as k_distance_within (withinTileWalk), but a pair that is linked keeps its
//                      `differing` and every other cell is UINT32_MAX (silo_gpu_distance_weights); a tile writes its transpose too
//   k_distance_listed_pairs  a wave per pair of a list of keys: both counts of the pairs a spanning forest kept
//                      (silo_gpu_distance_listed_pairs)
// and as a rectangle, one set of rows against another, behind NearestAmong (K14):
//   k_distance_cross   the same walk over the plain grid of 16 x 64 tiles of n_rows x n_columns pairs, each side with a plane buffer
//                      of its own; a pair that is eligible keeps both counts and every other cell is (UINT32_MAX, UINT32_MAX)
//                      (silo_gpu_distance_cross)
#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t DISTANCE_THREADS = 256;
constexpr uint32_t DISTANCE_TILE = SILO_GPU_DISTANCE_TILE;                // rows per side of a block's tile: one pair per thread
constexpr uint32_t DISTANCE_CHUNK_WORDS = SILO_GPU_DISTANCE_CHUNK_WORDS;  // words of every plane of a row that are staged at a time
constexpr uint32_t DISTANCE_PACK_WAVES = DISTANCE_THREADS / 64;           // words of a row per block of k_distance_pack
constexpr uint8_t NOT_VALID = 0xFF;
static_assert(DISTANCE_TILE * DISTANCE_TILE == DISTANCE_THREADS);
constexpr uint32_t WITHIN_TILE_ROWS = SILO_GPU_WITHIN_TILE_ROWS;      // rows of a block's tile: WITHIN_ROWS_PER_WAVE per wave
constexpr uint32_t WITHIN_TILE_COLS = SILO_GPU_WITHIN_TILE_COLS;      // columns of a block's tile: one per lane, one adjacency word
constexpr uint32_t WITHIN_CHUNK_WORDS = SILO_GPU_WITHIN_CHUNK_WORDS;  // words of every plane of a row that are staged at a time
constexpr uint32_t WITHIN_ROWS_PER_WAVE = WITHIN_TILE_ROWS / (DISTANCE_THREADS / 64u);  // pairs per thread
constexpr uint32_t WITHIN_ROW_TILES_PER_WORD = WITHIN_TILE_COLS / WITHIN_TILE_ROWS;     // row tiles that share a diagonal word
static_assert(WITHIN_TILE_COLS == 64 && WITHIN_ROWS_PER_WAVE * (DISTANCE_THREADS / 64u) == WITHIN_TILE_ROWS);
static_assert(WITHIN_ROW_TILES_PER_WORD * WITHIN_TILE_ROWS == WITHIN_TILE_COLS);

/// The valid mutation symbols of an alphabet as characters, in the order of Nucleotide / AminoAcid::VALID_MUTATION_SYMBOLS
/// (host/symbols.h): the index of a character in here is the code the planes hold.
struct DistanceSymbols {
   char symbols[24];
   uint32_t count;
};

constexpr DistanceSymbols NUCLEOTIDE_SYMBOLS{"-ACGT", 5};
constexpr DistanceSymbols AMINO_ACID_SYMBOLS{"-ACDEFGHIKLMNPQRSTVWY*", 22};
static_assert((1u << (SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE) - 1u)) >= NUCLEOTIDE_SYMBOLS.count);
static_assert((1u << (SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID) - 1u)) >= AMINO_ACID_SYMBOLS.count);

/// grid = (words of a row / DISTANCE_PACK_WAVES rounded up, n_rows).  The block first makes the table byte -> code (the index
/// among the valid symbols, NOT_VALID for every other byte, one entry per thread); then wave v takes word blockIdx.x *
/// DISTANCE_PACK_WAVES + v of row blockIdx.y: lane l reads the character at position 64 * word + l — a lane at or past
/// `positions` reads nothing and counts as not valid, so the padding bits of the last word are zero — and the ballots over the
/// wave are the word of plane 0 (valid) and of planes 1 .. PLANES - 1 (bit k - 1 of the code).  Lane 0 stores them.
template <uint32_t PLANES>
__global__ __launch_bounds__(DISTANCE_THREADS) void k_distance_pack(
   const DistanceSymbols valid, const uint8_t* __restrict__ chars, uint32_t positions, uint32_t words, uint64_t* __restrict__ planes
) {
   __shared__ uint8_t s_code[256];
   {
      uint8_t code = NOT_VALID;
      for (uint32_t s = 0; s < valid.count; ++s) {
         if (static_cast<uint8_t>(valid.symbols[s]) == threadIdx.x) {
            code = static_cast<uint8_t>(s);
         }
      }
      s_code[threadIdx.x] = code;
   }
   __syncthreads();
   const uint32_t word = blockIdx.x * DISTANCE_PACK_WAVES + threadIdx.x / 64u;  // the same for the whole wave
   if (word >= words) {
      return;
   }
   const uint32_t row = blockIdx.y;
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t position = static_cast<uint64_t>(word) * 64u + lane;
   uint8_t code = NOT_VALID;
   if (position < positions) {
      code = s_code[chars[static_cast<size_t>(row) * positions + position]];
   }
   const bool is_valid = code != NOT_VALID;
   uint64_t bits[PLANES];
   bits[0] = __ballot(is_valid);
#pragma unroll
   for (uint32_t k = 1; k < PLANES; ++k) {
      bits[k] = __ballot(is_valid && ((code >> (k - 1u)) & 1u) != 0);
   }
   if (lane == 0) {
      uint64_t* slot = planes + static_cast<size_t>(row) * PLANES * words + word;
#pragma unroll
      for (uint32_t k = 0; k < PLANES; ++k) {
         slot[static_cast<size_t>(k) * words] = bits[k];
      }
   }
}

/// A row of the staged tile in LDS: DISTANCE_CHUNK_WORDS words of each plane, and one word of padding — the 16 rows that the
/// lanes of a half wave read at the same (plane, word) then lie on 16 different bank pairs.
template <uint32_t PLANES>
constexpr uint32_t stagedRowWords() {
   return PLANES * DISTANCE_CHUNK_WORDS + 1u;
}

/// grid = the tiles (ti, tj), ti <= tj, of the upper triangle, row-major: tiles_per_side * (tiles_per_side + 1) / 2 blocks.
/// Thread t owns the pair (row ti * TILE + t / TILE, row tj * TILE + t % TILE).  Per chunk of DISTANCE_CHUNK_WORDS words the
/// block copies the words of all planes of its 2 x TILE rows into LDS — consecutive threads take consecutive words of one plane
/// of one row; a row at or past n_rows is staged as zeros, so nothing past the buffer is read — and every thread walks the
/// chunk: the lanes that share a row of the first side read the same LDS address (broadcast).  Two register accumulators per
/// thread; the pair's cell is written once at the end, and only where i <= j < n_rows.
template <uint32_t PLANES>
__global__ __launch_bounds__(DISTANCE_THREADS) void k_distance_pairs(
   const uint64_t* __restrict__ planes, uint32_t n_rows, uint32_t words, uint32_t tiles_per_side, uint32_t* __restrict__ out
) {
   constexpr uint32_t ROW_WORDS = stagedRowWords<PLANES>();
   constexpr uint32_t STAGED = 2u * DISTANCE_TILE * PLANES * DISTANCE_CHUNK_WORDS;  // words copied per chunk
   static_assert(STAGED % DISTANCE_THREADS == 0);
   __shared__ uint64_t s_rows[2u * DISTANCE_TILE * ROW_WORDS];

   // the tile of this block: row ti of the triangle has tiles_per_side - ti tiles (uniform, at most tiles_per_side steps)
   uint32_t ti = 0;
   uint32_t tj = blockIdx.x;
   for (uint32_t row_tiles = tiles_per_side; tj >= row_tiles; --row_tiles) {
      tj -= row_tiles;
      ++ti;
   }
   tj += ti;
   const uint32_t i = threadIdx.x / DISTANCE_TILE;
   const uint32_t j = threadIdx.x % DISTANCE_TILE;
   const uint64_t* mine = s_rows + i * ROW_WORDS;
   const uint64_t* other = s_rows + (DISTANCE_TILE + j) * ROW_WORDS;
   uint32_t compared = 0;
   uint32_t differing = 0;
   for (uint32_t chunk_begin = 0; chunk_begin < words; chunk_begin += DISTANCE_CHUNK_WORDS) {
      const uint32_t chunk_words = min(words - chunk_begin, DISTANCE_CHUNK_WORDS);
      uint64_t staged[STAGED / DISTANCE_THREADS];
#pragma unroll
      for (uint32_t k = 0; k < STAGED / DISTANCE_THREADS; ++k) {  // all loads in flight
         const uint32_t element = k * DISTANCE_THREADS + threadIdx.x;
         const uint32_t word = element % DISTANCE_CHUNK_WORDS;
         const uint32_t row_plane = element / DISTANCE_CHUNK_WORDS;  // (side * TILE + row of the side) * PLANES + plane
         const uint32_t local_row = row_plane / PLANES;
         const uint32_t row = local_row < DISTANCE_TILE ? ti * DISTANCE_TILE + local_row : tj * DISTANCE_TILE + (local_row - DISTANCE_TILE);
         staged[k] = 0;
         if (row < n_rows && word < chunk_words) {
            staged[k] = planes[(static_cast<size_t>(row) * PLANES + row_plane % PLANES) * words + chunk_begin + word];
         }
      }
#pragma unroll
      for (uint32_t k = 0; k < STAGED / DISTANCE_THREADS; ++k) {
         const uint32_t element = k * DISTANCE_THREADS + threadIdx.x;
         const uint32_t row_plane = element / DISTANCE_CHUNK_WORDS;
         s_rows[(row_plane / PLANES) * ROW_WORDS + (row_plane % PLANES) * DISTANCE_CHUNK_WORDS + element % DISTANCE_CHUNK_WORDS] = staged[k];
      }
      __syncthreads();
      for (uint32_t word = 0; word < chunk_words; ++word) {
         const uint64_t both = mine[word] & other[word];
         uint64_t unequal = 0;
#pragma unroll
         for (uint32_t k = 1; k < PLANES; ++k) {
            unequal |= mine[k * DISTANCE_CHUNK_WORDS + word] ^ other[k * DISTANCE_CHUNK_WORDS + word];
         }
         compared += static_cast<uint32_t>(__popcll(both));
         differing += static_cast<uint32_t>(__popcll(both & unequal));
      }
      __syncthreads();  // the next chunk overwrites what was just read
   }
   const uint32_t row_i = ti * DISTANCE_TILE + i;
   const uint32_t row_j = tj * DISTANCE_TILE + j;
   if (row_i <= row_j && row_j < n_rows) {
      *reinterpret_cast<uint2*>(out + (static_cast<size_t>(row_i) * n_rows + row_j) * 2u) = make_uint2(differing, compared);
   }
}

/// A row of the tile that k_distance_within stages: WITHIN_CHUNK_WORDS words of each plane, and one word of padding.  The stride
/// is an odd number of 8-byte words, so the 32 lanes that an 8-byte LDS read serves together, which read 32 consecutive rows at
/// the same (plane, word), fall on 32 different pairs of banks.
template <uint32_t PLANES>
constexpr uint32_t withinRowWords() {
   return PLANES * WITHIN_CHUNK_WORDS + 1u;
}
static_assert(withinRowWords<4>() % 2u == 1u && withinRowWords<6>() % 2u == 1u);

/// The tile (ti, tj) of block `index` among the tiles with tj >= the word of the diagonal of row tile ti, row tile by row tile: the
/// row tiles 4 g .. 4 g + 3 (WITHIN_ROW_TILES_PER_WORD of them share the diagonal word g) have adjacency_words - g tiles each.
/// Uniform over the block, at most adjacency_words steps.
__device__ __forceinline__ void withinTileOf(uint32_t index, uint32_t row_tiles, uint32_t adjacency_words, uint32_t& ti, uint32_t& tj) {
   ti = 0;
   tj = 0;
   for (uint32_t group = 0; group < adjacency_words; ++group) {
      const uint32_t tiles_per_row_tile = adjacency_words - group;
      const uint32_t group_row_tiles = min(WITHIN_ROW_TILES_PER_WORD, row_tiles - group * WITHIN_ROW_TILES_PER_WORD);
      if (index < group_row_tiles * tiles_per_row_tile) {
         ti = group * WITHIN_ROW_TILES_PER_WORD + index / tiles_per_row_tile;
         tj = group + index % tiles_per_row_tile;
         break;
      }
      index -= group_row_tiles * tiles_per_row_tile;
   }
}

/// The pairs of one thread of a WITHIN_TILE_ROWS x WITHIN_TILE_COLS tile: its column against its wave's four rows.
struct WithinPairs {
   uint32_t compared[WITHIN_ROWS_PER_WAVE];
   uint32_t differing[WITHIN_ROWS_PER_WAVE];
   bool open[WITHIN_ROWS_PER_WAVE];  // still linkable: the caller's start (row and column in range, not the same row), then differing <= max_distance so far
};

/// Where the pairs of this thread start: in range on both sides and not what `excluded(row, column)` names.
template <typename Excluded>
__device__ __forceinline__ void withinOpen(WithinPairs& pairs, uint32_t ti, uint32_t tj, uint32_t n_rows, uint32_t n_columns, Excluded excluded) {
   const uint32_t first_row = ti * WITHIN_TILE_ROWS + (threadIdx.x / 64u) * WITHIN_ROWS_PER_WAVE;
   const uint32_t column = tj * WITHIN_TILE_COLS + (threadIdx.x & 63u);
#pragma unroll
   for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
      pairs.open[r] = first_row + r < n_rows && column < n_columns && !excluded(first_row + r, column);
   }
}

/// The walk of tile (ti, tj) that k_distance_within, k_distance_weights and k_distance_cross share; the whole block calls it, s_rows
/// is its LDS of (WITHIN_TILE_ROWS + WITHIN_TILE_COLS) * withinRowWords<PLANES>() words.  The row side (row_planes, n_rows) and the
/// column side (column_planes, n_columns) each have a plane buffer and a row count of their own; the square kernels pass the same
/// buffer and count twice.  Wave v owns rows ti * 16 + 4 v .. + 3 of the tile, lane l its column tj * 64 + l.  Per chunk of
/// WITHIN_CHUNK_WORDS words the block copies the words of all planes of its 16 + 64 rows into LDS — a row at or past its side's
/// count is staged as zeros, so nothing past either buffer is read — and every thread walks the chunk with its column's words (one
/// LDS read per plane and word) against its four rows' (the same address for the whole wave: broadcast).  The CALLER sets
/// pairs.open before the walk (withinOpen): a pair is `open` while it can still be linked — never a pair with a row at or past
/// n_rows, a column at or past n_columns or the caller's own exclusion (i == j, self[i] == j), and no longer once differing >
/// max_distance.  The walk clears the two counts.  After each chunk the block leaves the loop if no pair is open.  Every path out of
/// here ends with a barrier after the last read of s_rows (or never touched it): the caller may reuse it at once.
template <uint32_t PLANES>
__device__ __forceinline__ void withinTileWalk(
   const uint64_t* __restrict__ row_planes, uint32_t n_rows, const uint64_t* __restrict__ column_planes, uint32_t n_columns, uint32_t words,
   uint32_t ti, uint32_t tj, uint32_t max_distance, uint64_t* s_rows, WithinPairs& pairs
) {
   constexpr uint32_t ROW_WORDS = withinRowWords<PLANES>();
   constexpr uint32_t STAGED_ROWS = WITHIN_TILE_ROWS + WITHIN_TILE_COLS;
   constexpr uint32_t STAGED = STAGED_ROWS * PLANES * WITHIN_CHUNK_WORDS;  // words copied per chunk
   static_assert(STAGED % DISTANCE_THREADS == 0);
   const uint32_t wave = threadIdx.x / 64u;
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t* mine = s_rows + wave * WITHIN_ROWS_PER_WAVE * ROW_WORDS;
   const uint64_t* other = s_rows + (WITHIN_TILE_ROWS + lane) * ROW_WORDS;
   uint32_t (&compared)[WITHIN_ROWS_PER_WAVE] = pairs.compared;
   uint32_t (&differing)[WITHIN_ROWS_PER_WAVE] = pairs.differing;
   bool (&open)[WITHIN_ROWS_PER_WAVE] = pairs.open;
#pragma unroll
   for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
      compared[r] = 0;
      differing[r] = 0;
   }
   for (uint32_t chunk_begin = 0; chunk_begin < words; chunk_begin += WITHIN_CHUNK_WORDS) {
      const uint32_t chunk_words = min(words - chunk_begin, WITHIN_CHUNK_WORDS);
      uint64_t staged[STAGED / DISTANCE_THREADS];
#pragma unroll
      for (uint32_t k = 0; k < STAGED / DISTANCE_THREADS; ++k) {  // all loads in flight
         const uint32_t element = k * DISTANCE_THREADS + threadIdx.x;
         const uint32_t word = element % WITHIN_CHUNK_WORDS;
         const uint32_t row_plane = element / WITHIN_CHUNK_WORDS;  // (row of the tile's 16, then column of its 64) * PLANES + plane
         const uint32_t local_row = row_plane / PLANES;
         const bool row_side = local_row < WITHIN_TILE_ROWS;
         const uint32_t row = row_side ? ti * WITHIN_TILE_ROWS + local_row : tj * WITHIN_TILE_COLS + (local_row - WITHIN_TILE_ROWS);
         staged[k] = 0;
         if (row < (row_side ? n_rows : n_columns) && word < chunk_words) {
            staged[k] = (row_side ? row_planes : column_planes)[(static_cast<size_t>(row) * PLANES + row_plane % PLANES) * words + chunk_begin + word];
         }
      }
#pragma unroll
      for (uint32_t k = 0; k < STAGED / DISTANCE_THREADS; ++k) {
         const uint32_t element = k * DISTANCE_THREADS + threadIdx.x;
         const uint32_t row_plane = element / WITHIN_CHUNK_WORDS;
         s_rows[(row_plane / PLANES) * ROW_WORDS + (row_plane % PLANES) * WITHIN_CHUNK_WORDS + element % WITHIN_CHUNK_WORDS] = staged[k];
      }
      __syncthreads();
      for (uint32_t word = 0; word < chunk_words; ++word) {
         uint64_t theirs[PLANES];
#pragma unroll
         for (uint32_t k = 0; k < PLANES; ++k) {
            theirs[k] = other[k * WITHIN_CHUNK_WORDS + word];
         }
#pragma unroll
         for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
            const uint64_t* row = mine + r * ROW_WORDS;
            const uint64_t both = row[word] & theirs[0];
            uint64_t unequal = 0;
#pragma unroll
            for (uint32_t k = 1; k < PLANES; ++k) {
               unequal |= row[k * WITHIN_CHUNK_WORDS + word] ^ theirs[k];
            }
            compared[r] += static_cast<uint32_t>(__popcll(both));
            differing[r] += static_cast<uint32_t>(__popcll(both & unequal));
         }
      }
      bool any_open = false;
#pragma unroll
      for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
         open[r] = open[r] && differing[r] <= max_distance;
         any_open = any_open || open[r];
      }
      // the barrier that lets the next chunk overwrite what was just read, and the vote: differing only grows along the row
      if (__syncthreads_or(any_open) == 0) {
         break;
      }
   }
}

/// grid = the tiles of withinTileOf.  After the walk the ballot of "open and compared >= min_compared" over a wave is word (row, tj);
/// one lane stores it, for rows < n_rows.
template <uint32_t PLANES>
__global__ __launch_bounds__(DISTANCE_THREADS) void k_distance_within(
   const uint64_t* __restrict__ planes, uint32_t n_rows, uint32_t words, uint32_t row_tiles, uint32_t adjacency_words, uint32_t max_distance,
   uint32_t min_compared, uint64_t* __restrict__ adjacency
) {
   __shared__ uint64_t s_rows[(WITHIN_TILE_ROWS + WITHIN_TILE_COLS) * withinRowWords<PLANES>()];
   uint32_t ti;
   uint32_t tj;
   withinTileOf(blockIdx.x, row_tiles, adjacency_words, ti, tj);
   WithinPairs pairs;
   withinOpen(pairs, ti, tj, n_rows, n_rows, [](uint32_t i, uint32_t j) { return i == j; });
   withinTileWalk<PLANES>(planes, n_rows, planes, n_rows, words, ti, tj, max_distance, s_rows, pairs);
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t first_row = ti * WITHIN_TILE_ROWS + (threadIdx.x / 64u) * WITHIN_ROWS_PER_WAVE;
#pragma unroll
   for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
      const uint64_t linked = __ballot(pairs.open[r] && pairs.differing[r] <= max_distance && pairs.compared[r] >= min_compared);
      if (lane == 0 && first_row + r < n_rows) {
         adjacency[static_cast<size_t>(first_row + r) * adjacency_words + tj] = linked;
      }
   }
}

/// A row of the tile of weights that k_distance_weights transposes through LDS: WITHIN_TILE_COLS cells and one of padding, so the
/// 16 cells of a column that consecutive lanes read lie in different banks.
constexpr uint32_t WEIGHTS_TILE_STRIDE = WITHIN_TILE_COLS + 1u;
static_assert(WITHIN_TILE_ROWS * WEIGHTS_TILE_STRIDE * sizeof(uint32_t) <= (WITHIN_TILE_ROWS + WITHIN_TILE_COLS) * withinRowWords<4>() * sizeof(uint64_t));

/// grid = the tiles of withinTileOf, the walk of withinTileWalk.  Afterwards a pair's cell is its `differing` if it is an edge (open,
/// differing <= max_distance, compared >= min_compared) and UINT32_MAX if not — the diagonal and the pairs of a block that stopped
/// early included.  Every thread stores its four cells (row, column) where both are < n_rows: consecutive lanes, consecutive cells.
/// A tile right of the diagonal's 64 x 64 block also owns the transposed cells (column, row), which no launched tile covers: the
/// cells go through LDS (s_rows is free after the walk) and 16 consecutive threads store the 16 consecutive cells of a column.
/// The four row tiles of the diagonal's block cover both halves of it themselves.  So every cell has one writer.
template <uint32_t PLANES>
__global__ __launch_bounds__(DISTANCE_THREADS) void k_distance_weights(
   const uint64_t* __restrict__ planes, uint32_t n_rows, uint32_t words, uint32_t row_tiles, uint32_t adjacency_words, uint32_t max_distance,
   uint32_t min_compared, uint32_t* __restrict__ weights
) {
   __shared__ uint64_t s_rows[(WITHIN_TILE_ROWS + WITHIN_TILE_COLS) * withinRowWords<PLANES>()];
   uint32_t ti;
   uint32_t tj;
   withinTileOf(blockIdx.x, row_tiles, adjacency_words, ti, tj);
   WithinPairs pairs;
   withinOpen(pairs, ti, tj, n_rows, n_rows, [](uint32_t i, uint32_t j) { return i == j; });
   withinTileWalk<PLANES>(planes, n_rows, planes, n_rows, words, ti, tj, max_distance, s_rows, pairs);
   const uint32_t wave = threadIdx.x / 64u;
   const uint32_t lane = threadIdx.x & 63u;
   const uint32_t first_row = ti * WITHIN_TILE_ROWS + wave * WITHIN_ROWS_PER_WAVE;
   const uint32_t column = tj * WITHIN_TILE_COLS + lane;
   const bool mirrored = tj > ti / WITHIN_ROW_TILES_PER_WORD;  // uniform
   auto* s_tile = reinterpret_cast<uint32_t*>(s_rows);
#pragma unroll
   for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
      const bool edge = pairs.open[r] && pairs.differing[r] <= max_distance && pairs.compared[r] >= min_compared;
      const uint32_t weight = edge ? pairs.differing[r] : UINT32_MAX;
      if (first_row + r < n_rows && column < n_rows) {
         weights[static_cast<size_t>(first_row + r) * n_rows + column] = weight;
      }
      if (mirrored) {
         s_tile[(wave * WITHIN_ROWS_PER_WAVE + r) * WEIGHTS_TILE_STRIDE + lane] = weight;
      }
   }
   if (!mirrored) {
      return;
   }
   __syncthreads();
#pragma unroll
   for (uint32_t k = 0; k < WITHIN_TILE_ROWS * WITHIN_TILE_COLS / DISTANCE_THREADS; ++k) {
      const uint32_t cell = k * DISTANCE_THREADS + threadIdx.x;
      const uint32_t tile_row = cell % WITHIN_TILE_ROWS;
      const uint32_t tile_column = cell / WITHIN_TILE_ROWS;
      const uint32_t row = ti * WITHIN_TILE_ROWS + tile_row;
      const uint32_t mirrored_row = tj * WITHIN_TILE_COLS + tile_column;
      if (row < n_rows && mirrored_row < n_rows) {
         weights[static_cast<size_t>(mirrored_row) * n_rows + row] = s_tile[tile_row * WEIGHTS_TILE_STRIDE + tile_column];
      }
   }
}

/// grid = (n_columns / 64 rounded up, n_rows / 16 rounded up): the plain rectangle, no symmetry and no transpose.  self_column
/// (NULL: none) names per row the column that is the same database row; a value at or past n_columns excludes nothing.  After the
/// walk a pair's cell is (differing, compared) if it is eligible (open, differing <= max_distance, compared >= min_compared) and
/// (UINT32_MAX, UINT32_MAX) if not — self and the pairs of a block that stopped early included.  Every thread stores its four cells
/// (row, column) where row < n_rows and column < n_columns as 8-byte stores: consecutive lanes, consecutive cells.
template <uint32_t PLANES>
__global__ __launch_bounds__(DISTANCE_THREADS) void k_distance_cross(
   const uint64_t* __restrict__ row_planes, uint32_t n_rows, const uint64_t* __restrict__ column_planes, uint32_t n_columns, uint32_t words,
   const uint32_t* __restrict__ self_column, uint32_t max_distance, uint32_t min_compared, uint32_t* __restrict__ cells
) {
   __shared__ uint64_t s_rows[(WITHIN_TILE_ROWS + WITHIN_TILE_COLS) * withinRowWords<PLANES>()];
   const uint32_t ti = blockIdx.y;
   const uint32_t tj = blockIdx.x;
   const uint32_t first_row = ti * WITHIN_TILE_ROWS + (threadIdx.x / 64u) * WITHIN_ROWS_PER_WAVE;
   const uint32_t column = tj * WITHIN_TILE_COLS + (threadIdx.x & 63u);
   uint32_t self[WITHIN_ROWS_PER_WAVE];
#pragma unroll
   for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
      self[r] = self_column != nullptr && first_row + r < n_rows ? self_column[first_row + r] : UINT32_MAX;
   }
   WithinPairs pairs;
   withinOpen(pairs, ti, tj, n_rows, n_columns, [&](uint32_t i, uint32_t j) { return self[i - first_row] == j; });
   withinTileWalk<PLANES>(row_planes, n_rows, column_planes, n_columns, words, ti, tj, max_distance, s_rows, pairs);
#pragma unroll
   for (uint32_t r = 0; r < WITHIN_ROWS_PER_WAVE; ++r) {
      const bool eligible = pairs.open[r] && pairs.differing[r] <= max_distance && pairs.compared[r] >= min_compared;
      if (first_row + r < n_rows && column < n_columns) {
         *reinterpret_cast<uint2*>(cells + (static_cast<size_t>(first_row + r) * n_columns + column) * 2u) =
            eligible ? make_uint2(pairs.differing[r], pairs.compared[r]) : make_uint2(UINT32_MAX, UINT32_MAX);
      }
   }
}

/// grid = max_pairs / 4 rounded up, a wave per listed pair e < min(*count, max_pairs): (i, j) from the low 26 bits of keys[e]; a
/// key that names a row at or past n_rows gets (UINT32_MAX, UINT32_MAX) and reads no plane.  Lane l takes the words l, l + 64, ...
/// of the two rows, one reduction over the wave, lane 0 stores the two counts.
template <uint32_t PLANES>
__global__ __launch_bounds__(DISTANCE_THREADS) void k_distance_listed_pairs(
   const uint64_t* __restrict__ planes, uint32_t n_rows, uint32_t words, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ count,
   uint32_t max_pairs, uint32_t* __restrict__ out
) {
   const uint32_t pair = blockIdx.x * (DISTANCE_THREADS / 64u) + threadIdx.x / 64u;  // the same for the whole wave
   if (pair >= min(*count, max_pairs)) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t key = keys[pair];
   const uint32_t i = static_cast<uint32_t>(key >> SILO_GPU_SPANNING_KEY_ROW_BITS) & (SILO_GPU_MAX_SPANNING_ROWS - 1u);
   const uint32_t j = static_cast<uint32_t>(key) & (SILO_GPU_MAX_SPANNING_ROWS - 1u);
   uint32_t compared = UINT32_MAX;
   uint32_t differing = UINT32_MAX;
   if (i < n_rows && j < n_rows) {
      const uint64_t* mine = planes + static_cast<size_t>(i) * PLANES * words;
      const uint64_t* other = planes + static_cast<size_t>(j) * PLANES * words;
      compared = 0;
      differing = 0;
      for (uint32_t word = lane; word < words; word += 64u) {
         const uint64_t both = mine[word] & other[word];
         uint64_t unequal = 0;
#pragma unroll
         for (uint32_t k = 1; k < PLANES; ++k) {
            unequal |= mine[static_cast<size_t>(k) * words + word] ^ other[static_cast<size_t>(k) * words + word];
         }
         compared += static_cast<uint32_t>(__popcll(both));
         differing += static_cast<uint32_t>(__popcll(both & unequal));
      }
#pragma unroll
      for (uint32_t offset = 32; offset > 0; offset >>= 1) {
         compared += static_cast<uint32_t>(__shfl_xor(static_cast<int>(compared), static_cast<int>(offset)));
         differing += static_cast<uint32_t>(__shfl_xor(static_cast<int>(differing), static_cast<int>(offset)));
      }
   }
   if (lane == 0) {
      out[static_cast<size_t>(pair) * 2u] = differing;
      out[static_cast<size_t>(pair) * 2u + 1u] = compared;
   }
}

/// grid = (adjacency_words / 4 rounded up, adjacency_words), a wave per 64 x 64 bit block (wi, wj) with wj < wi, the blocks left of
/// the diagonal's: lane l reads word (64 wj + l, wi) — right of its row's diagonal word, so k_distance_within wrote it, and
/// 64 wj + l < 64 wi < n_rows — the ballot of bit b over the wave is word (64 wi + b, wj), which lane b keeps and stores where its
/// row is < n_rows.  Reads words right of the diagonal only and writes words left of it only.
__global__ __launch_bounds__(DISTANCE_THREADS) void k_adjacency_mirror(uint64_t* adjacency, uint32_t n_rows, uint32_t adjacency_words) {
   const uint32_t wi = blockIdx.y;
   const uint32_t wj = blockIdx.x * (DISTANCE_THREADS / 64u) + threadIdx.x / 64u;  // the same for the whole wave
   if (wj >= wi) {
      return;
   }
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t column_bits = adjacency[static_cast<size_t>(wj * 64u + lane) * adjacency_words + wi];
   uint64_t row_bits = 0;
   for (uint32_t bit = 0; bit < 64u; ++bit) {
      const uint64_t transposed = __ballot(((column_bits >> bit) & 1u) != 0);
      if (lane == bit) {
         row_bits = transposed;
      }
   }
   const uint32_t row = wi * 64u + lane;
   if (row < n_rows) {
      adjacency[static_cast<size_t>(row) * adjacency_words + wj] = row_bits;
   }
}

constexpr const char* MORE_THAN_DISTANCE_ROWS = "more rows than SILO_GPU_MAX_DISTANCE_ROWS";
constexpr const char* MORE_THAN_CLUSTER_ROWS = "more rows than SILO_GPU_MAX_CLUSTER_ROWS";
constexpr const char* MORE_THAN_SPANNING_ROWS = "more rows than SILO_GPU_MAX_SPANNING_ROWS";
static_assert(SILO_GPU_MAX_SPANNING_ROWS == SILO_GPU_MAX_CLUSTER_ROWS && SILO_GPU_MAX_SPANNING_ROWS == 1u << SILO_GPU_SPANNING_KEY_ROW_BITS);
static_assert(SILO_GPU_MAX_CROSS_ROWS == SILO_GPU_MAX_DISTANCE_ROWS && SILO_GPU_MAX_CROSS_COLUMNS == SILO_GPU_MAX_CLUSTER_ROWS);

/// Blocks of k_distance_within / k_distance_weights: the tiles withinTileOf numbers.
uint32_t withinTiles(uint32_t row_tiles, uint32_t adjacency_words) {
   uint32_t grid = 0;
   for (uint32_t group = 0; group < adjacency_words; ++group) {
      grid += std::min(WITHIN_ROW_TILES_PER_WORD, row_tiles - group * WITHIN_ROW_TILES_PER_WORD) * (adjacency_words - group);
   }
   return grid;
}

/// What the entries refuse; nullptr if nothing.  limit_complaint: what to say of more than max_rows rows.
const char* distanceComplaint(int alphabet, const void* in_dev, const void* out_dev, uint32_t n_rows, uint32_t max_rows, const char* limit_complaint) {
   if (alphabet != SILO_GPU_ALPHABET_NUCLEOTIDE && alphabet != SILO_GPU_ALPHABET_AMINO_ACID) {
      return "the alphabet is neither SILO_GPU_ALPHABET_NUCLEOTIDE nor SILO_GPU_ALPHABET_AMINO_ACID";
   }
   if (in_dev == nullptr || out_dev == nullptr) {
      return "a buffer is NULL";
   }
   if (n_rows > max_rows) {
      return limit_complaint;
   }
   return nullptr;
}

}  // namespace

extern "C" {

int silo_gpu_distance_pack(int alphabet, const char* chars_dev, uint32_t n_rows, uint32_t positions, uint64_t* planes_dev, void* stream) {
   if (const char* complaint = distanceComplaint(alphabet, chars_dev, planes_dev, n_rows, SILO_GPU_MAX_DISTANCE_ROWS, MORE_THAN_DISTANCE_ROWS); complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_distance_pack: ") + complaint);
   }
   if (n_rows == 0 || positions == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t words = SILO_GPU_DISTANCE_WORDS(positions);
   const dim3 grid((words + DISTANCE_PACK_WAVES - 1) / DISTANCE_PACK_WAVES, n_rows);
   auto hip_stream = static_cast<hipStream_t>(stream);
   const auto* chars = reinterpret_cast<const uint8_t*>(chars_dev);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_distance_pack<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE)>
         <<<grid, DISTANCE_THREADS, 0, hip_stream>>>(NUCLEOTIDE_SYMBOLS, chars, positions, words, planes_dev);
   } else {
      k_distance_pack<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID)>
         <<<grid, DISTANCE_THREADS, 0, hip_stream>>>(AMINO_ACID_SYMBOLS, chars, positions, words, planes_dev);
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distance_pairs(int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, uint32_t* out_dev, void* stream) {
   if (const char* complaint = distanceComplaint(alphabet, planes_dev, out_dev, n_rows, SILO_GPU_MAX_DISTANCE_ROWS, MORE_THAN_DISTANCE_ROWS); complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_distance_pairs: ") + complaint);
   }
   if (n_rows == 0 || positions == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t words = SILO_GPU_DISTANCE_WORDS(positions);
   const uint32_t tiles_per_side = (n_rows + DISTANCE_TILE - 1) / DISTANCE_TILE;
   const uint32_t grid = tiles_per_side * (tiles_per_side + 1u) / 2u;
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_distance_pairs<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE)>
         <<<grid, DISTANCE_THREADS, 0, hip_stream>>>(planes_dev, n_rows, words, tiles_per_side, out_dev);
   } else {
      k_distance_pairs<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID)>
         <<<grid, DISTANCE_THREADS, 0, hip_stream>>>(planes_dev, n_rows, words, tiles_per_side, out_dev);
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distance_within(
   int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, uint32_t max_distance, uint32_t min_compared,
   uint64_t* adjacency_dev, void* stream
) {
   if (const char* complaint = distanceComplaint(alphabet, planes_dev, adjacency_dev, n_rows, SILO_GPU_MAX_CLUSTER_ROWS, MORE_THAN_CLUSTER_ROWS);
       complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_distance_within: ") + complaint);
   }
   if (n_rows == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t words = SILO_GPU_DISTANCE_WORDS(positions);  // 0 positions: no chunk is walked, every pair has (0, 0)
   const uint32_t adjacency_words = SILO_GPU_ADJACENCY_WORDS(n_rows);
   const uint32_t row_tiles = (n_rows + WITHIN_TILE_ROWS - 1) / WITHIN_TILE_ROWS;
   const uint32_t grid = withinTiles(row_tiles, adjacency_words);
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_distance_within<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE)><<<grid, DISTANCE_THREADS, 0, hip_stream>>>(
         planes_dev, n_rows, words, row_tiles, adjacency_words, max_distance, min_compared, adjacency_dev
      );
   } else {
      k_distance_within<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID)><<<grid, DISTANCE_THREADS, 0, hip_stream>>>(
         planes_dev, n_rows, words, row_tiles, adjacency_words, max_distance, min_compared, adjacency_dev
      );
   }
   HIP_TRY(hipGetLastError());
   if (adjacency_words > 1) {
      const dim3 mirror_grid((adjacency_words + DISTANCE_THREADS / 64u - 1) / (DISTANCE_THREADS / 64u), adjacency_words);
      k_adjacency_mirror<<<mirror_grid, DISTANCE_THREADS, 0, hip_stream>>>(adjacency_dev, n_rows, adjacency_words);
      HIP_TRY(hipGetLastError());
   }
   return SILO_GPU_OK;
}

int silo_gpu_distance_weights(
   int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, uint32_t max_distance, uint32_t min_compared,
   uint32_t* weights_dev, void* stream
) {
   if (const char* complaint = distanceComplaint(alphabet, planes_dev, weights_dev, n_rows, SILO_GPU_MAX_SPANNING_ROWS, MORE_THAN_SPANNING_ROWS);
       complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_distance_weights: ") + complaint);
   }
   if (n_rows == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t words = SILO_GPU_DISTANCE_WORDS(positions);  // 0 positions: no chunk is walked, every pair has (0, 0)
   const uint32_t adjacency_words = SILO_GPU_ADJACENCY_WORDS(n_rows);
   const uint32_t row_tiles = (n_rows + WITHIN_TILE_ROWS - 1) / WITHIN_TILE_ROWS;
   const uint32_t grid = withinTiles(row_tiles, adjacency_words);
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_distance_weights<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE)><<<grid, DISTANCE_THREADS, 0, hip_stream>>>(
         planes_dev, n_rows, words, row_tiles, adjacency_words, max_distance, min_compared, weights_dev
      );
   } else {
      k_distance_weights<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID)><<<grid, DISTANCE_THREADS, 0, hip_stream>>>(
         planes_dev, n_rows, words, row_tiles, adjacency_words, max_distance, min_compared, weights_dev
      );
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distance_cross(
   int alphabet, const uint64_t* row_planes_dev, uint32_t n_rows, const uint64_t* column_planes_dev, uint32_t n_columns, uint32_t positions,
   const uint32_t* self_column_dev, uint32_t max_distance, uint32_t min_compared, uint32_t* cells_dev, void* stream
) {
   if (const char* complaint = distanceComplaint(alphabet, row_planes_dev, cells_dev, n_rows, SILO_GPU_MAX_CROSS_ROWS, "more rows than SILO_GPU_MAX_CROSS_ROWS");
       complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_distance_cross: ") + complaint);
   }
   if (column_planes_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_distance_cross: a buffer is NULL");
   }
   if (n_columns > SILO_GPU_MAX_CROSS_COLUMNS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_distance_cross: more columns than SILO_GPU_MAX_CROSS_COLUMNS");
   }
   if (n_rows == 0 || n_columns == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t words = SILO_GPU_DISTANCE_WORDS(positions);  // 0 positions: no chunk is walked, every pair has (0, 0)
   const dim3 grid((n_columns + WITHIN_TILE_COLS - 1) / WITHIN_TILE_COLS, (n_rows + WITHIN_TILE_ROWS - 1) / WITHIN_TILE_ROWS);
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_distance_cross<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE)><<<grid, DISTANCE_THREADS, 0, hip_stream>>>(
         row_planes_dev, n_rows, column_planes_dev, n_columns, words, self_column_dev, max_distance, min_compared, cells_dev
      );
   } else {
      k_distance_cross<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID)><<<grid, DISTANCE_THREADS, 0, hip_stream>>>(
         row_planes_dev, n_rows, column_planes_dev, n_columns, words, self_column_dev, max_distance, min_compared, cells_dev
      );
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

int silo_gpu_distance_listed_pairs(
   int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, const uint64_t* edges_dev, const uint32_t* count_dev,
   uint32_t max_pairs, uint32_t* out_dev, void* stream
) {
   if (const char* complaint = distanceComplaint(alphabet, planes_dev, out_dev, n_rows, SILO_GPU_MAX_SPANNING_ROWS, MORE_THAN_SPANNING_ROWS);
       complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_distance_listed_pairs: ") + complaint);
   }
   if (edges_dev == nullptr || count_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_distance_listed_pairs: a buffer is NULL");
   }
   if (max_pairs == 0) {
      return SILO_GPU_OK;
   }
   const uint32_t words = SILO_GPU_DISTANCE_WORDS(positions);  // 0 positions: every listed pair has (0, 0)
   const uint32_t grid = (max_pairs + DISTANCE_THREADS / 64u - 1) / (DISTANCE_THREADS / 64u);
   auto hip_stream = static_cast<hipStream_t>(stream);
   if (alphabet == SILO_GPU_ALPHABET_NUCLEOTIDE) {
      k_distance_listed_pairs<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_NUCLEOTIDE)>
         <<<grid, DISTANCE_THREADS, 0, hip_stream>>>(planes_dev, n_rows, words, edges_dev, count_dev, max_pairs, out_dev);
   } else {
      k_distance_listed_pairs<SILO_GPU_DISTANCE_PLANES(SILO_GPU_ALPHABET_AMINO_ACID)>
         <<<grid, DISTANCE_THREADS, 0, hip_stream>>>(planes_dev, n_rows, words, edges_dev, count_dev, max_pairs, out_dev);
   }
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
