// silo_gpu_cross.hip — the pair count behind CrossTabulation (K9, silo_gpu_filters_cross): for two lists of row bitsets, the rows
// of a base filter that every pair (one of each list) has in common.  One launch on the caller's stream:
//   k_cross_filter_counts       an AND-popcount "GEMM" over bit rows: a block owns a chunk of row words and a tile of
//                               CROSS_TILE x CROSS_TILE pairs, reads each word of its 2 x CROSS_TILE bitsets once and adds its
//                               cells to the caller's table
#include <algorithm>
#include <vector>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

constexpr uint32_t CROSS_THREADS = 256;
constexpr uint32_t CROSS_TILE = SILO_GPU_CROSS_TILE;                // filters per side of a block's tile: 64 accumulators per thread
constexpr uint32_t CROSS_CHUNK_WORDS = SILO_GPU_CROSS_CHUNK_WORDS;  // row words per block
constexpr uint32_t CROSS_WORDS_PER_THREAD = CROSS_CHUNK_WORDS / CROSS_THREADS;
static_assert(CROSS_CHUNK_WORDS % CROSS_THREADS == 0 && CROSS_TILE * CROSS_TILE <= CROSS_THREADS);

/// The tables of a K9 launch (device pointers into the caller's scratch).  rows[i] / cols[j] = a row bitset of row_words words;
/// the entry has put the store's all-ones bitset where the caller passed NULL, so the kernel loads without asking.
struct CrossArgs {
   const uint64_t* base;          // nullptr = all rows
   const uint64_t* const* rows;   // [n_rows]
   const uint64_t* const* cols;   // [n_cols]
   const uint32_t* row_index;     // [n_rows] the table row of rows[i]
   const uint32_t* col_index;     // [n_cols] the table column of cols[j]
   uint32_t* out;                 // [out_rows][out_cols], accumulated into
   uint32_t n_rows;
   uint32_t n_cols;
   uint32_t out_cols;
   uint32_t row_words;
   uint32_t sequence_count;
};

// 8-byte load through a pointer that was itself read from memory (the table of bitsets): see loadGlobal16 (store_internal.h).
__device__ __forceinline__ uint64_t loadGlobal8(const uint64_t* ptr) {
   return *(const __attribute__((address_space(1))) uint64_t*)(ptr);
}

/// grid = (row_words / CROSS_CHUNK_WORDS rounded up, row tiles of CROSS_TILE, column tiles of CROSS_TILE).  A thread walks
/// CROSS_WORDS_PER_THREAD words of the chunk, a block's stride apart (coalesced across the wave; the bitset pointers are uniform).
/// Per word: the base word under the valid mask — a word without a row of the base reads no more —, the tile's row-filter words
/// ANDed with it, the column-filter words, and popcount(a_i & b_j) into 64 register accumulators.  A tile at the edge of a list
/// reads the tile's first bitset in place of the filters it does not have and counts them as zero words: nothing past the arrays
/// is read, and nothing is added for them.  At the end every accumulator is summed over the wave (DPP), over the block's waves
/// in LDS, and added to its cell if it is not zero.
__global__ __launch_bounds__(CROSS_THREADS) void k_cross_filter_counts(const CrossArgs args) {
   __shared__ uint32_t s_cells[CROSS_THREADS / 64][CROSS_TILE * CROSS_TILE];
   const uint32_t i_begin = blockIdx.y * CROSS_TILE;
   const uint32_t j_begin = blockIdx.z * CROSS_TILE;
   const uint32_t n_i = min(args.n_rows - i_begin, CROSS_TILE);  // (the grid has no block without a filter on either side)
   const uint32_t n_j = min(args.n_cols - j_begin, CROSS_TILE);
   const uint64_t* a_bits[CROSS_TILE];
   const uint64_t* b_bits[CROSS_TILE];
#pragma unroll
   for (uint32_t t = 0; t < CROSS_TILE; ++t) {
      a_bits[t] = args.rows[i_begin + (t < n_i ? t : 0u)];
      b_bits[t] = args.cols[j_begin + (t < n_j ? t : 0u)];
   }
   uint32_t acc[CROSS_TILE][CROSS_TILE];
#pragma unroll
   for (uint32_t i = 0; i < CROSS_TILE; ++i) {
#pragma unroll
      for (uint32_t j = 0; j < CROSS_TILE; ++j) {
         acc[i][j] = 0;
      }
   }
   const uint32_t chunk_begin = blockIdx.x * CROSS_CHUNK_WORDS;
#pragma unroll 1
   for (uint32_t k = 0; k < CROSS_WORDS_PER_THREAD; ++k) {
      const uint32_t word = chunk_begin + k * CROSS_THREADS + threadIdx.x;
      if (word >= args.row_words) {
         break;
      }
      const uint64_t base = (args.base != nullptr ? args.base[word] : ~0ull) & silo_gpu::valid_mask(word, args.sequence_count);
      if (base == 0) {
         continue;
      }
      uint64_t a[CROSS_TILE];
      uint64_t b[CROSS_TILE];
#pragma unroll
      for (uint32_t t = 0; t < CROSS_TILE; ++t) {  // 16 loads in flight
         a[t] = loadGlobal8(a_bits[t] + word);
         b[t] = loadGlobal8(b_bits[t] + word);
      }
#pragma unroll
      for (uint32_t t = 0; t < CROSS_TILE; ++t) {  // (uniform selects: the tile's extent is the block's)
         a[t] = t < n_i ? a[t] & base : 0ull;
         b[t] = t < n_j ? b[t] : 0ull;
      }
#pragma unroll
      for (uint32_t i = 0; i < CROSS_TILE; ++i) {
#pragma unroll
         for (uint32_t j = 0; j < CROSS_TILE; ++j) {
            acc[i][j] += static_cast<uint32_t>(__popcll(a[i] & b[j]));
         }
      }
   }
   __syncthreads();  // every lane is back: the wave sums below need whole waves
   const uint32_t wave = threadIdx.x / 64u;
   const bool last_lane = (threadIdx.x & 63u) == 63u;
#pragma unroll
   for (uint32_t i = 0; i < CROSS_TILE; ++i) {
#pragma unroll
      for (uint32_t j = 0; j < CROSS_TILE; ++j) {
         const uint32_t sum = waveSumToLane63(acc[i][j]);
         if (last_lane) {
            s_cells[wave][i * CROSS_TILE + j] = sum;
         }
      }
   }
   __syncthreads();
   if (threadIdx.x < CROSS_TILE * CROSS_TILE) {
      const uint32_t i = threadIdx.x / CROSS_TILE;
      const uint32_t j = threadIdx.x % CROSS_TILE;
      uint32_t count = 0;
#pragma unroll
      for (uint32_t w = 0; w < CROSS_THREADS / 64; ++w) {
         count += s_cells[w][threadIdx.x];
      }
      if (i < n_i && j < n_j && count != 0) {
         atomicAdd(args.out + static_cast<size_t>(args.row_index[i_begin + i]) * args.out_cols + args.col_index[j_begin + j], count);
      }
   }
}

/// Where the filters of one side land in the table: `index` (nullptr = identity) copied to `out`, each entry below `bound` and
/// given once.  Returns what is wrong with them, nullptr if nothing.
const char* landingIndex(const uint32_t* index, uint32_t n, uint32_t bound, uint32_t* out) {
   for (uint32_t k = 0; k < n; ++k) {
      out[k] = index != nullptr ? index[k] : k;
      if (out[k] >= bound) {
         return "an index is outside the table";
      }
   }
   std::vector<uint32_t> sorted(out, out + n);
   std::sort(sorted.begin(), sorted.end());
   if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
      return "an index is given twice";
   }
   return nullptr;
}

}  // namespace

extern "C" {

int silo_gpu_filters_cross(
   const silo_gpu_store* store, const uint64_t* base_filter_dev, const uint64_t* const* row_filters_dev, const uint32_t* row_index, uint32_t n_rows,
   const uint64_t* const* col_filters_dev, const uint32_t* col_index, uint32_t n_cols, void* scratch_dev, uint32_t* out_dev, uint32_t out_rows,
   uint32_t out_cols, void* stream
) {
   if (store == nullptr || scratch_dev == nullptr || out_dev == nullptr || row_filters_dev == nullptr || col_filters_dev == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_cross: bad arguments");
   }
   if (n_rows > SILO_GPU_MAX_CROSS_FILTERS || n_cols > SILO_GPU_MAX_CROSS_FILTERS) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_cross: too many filters on a side");
   }
   if (store->sequence_count == 0 || store->row_words == 0) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_cross: the store has no rows");
   }
   // what is uploaded: the filter pointers of both sides (all rows: the store's all-ones bitset), then where each lands in the table
   const uint32_t R = n_rows, C = n_cols;
   std::vector<uint64_t> tables(static_cast<size_t>(R) + C + (static_cast<size_t>(R) + C + 1u) / 2u, 0u);
   auto* t_row_index = reinterpret_cast<uint32_t*>(tables.data() + R + C);
   uint32_t* t_col_index = t_row_index + R;
   if (const char* complaint = landingIndex(row_index, R, out_rows, t_row_index); complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_filters_cross: rows: ") + complaint);
   }
   if (const char* complaint = landingIndex(col_index, C, out_cols, t_col_index); complaint != nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, std::string("silo_gpu_filters_cross: columns: ") + complaint);
   }
   if (R == 0 || C == 0) {
      return SILO_GPU_OK;
   }
   for (uint32_t i = 0; i < R; ++i) {
      tables[i] = reinterpret_cast<uint64_t>(row_filters_dev[i] != nullptr ? row_filters_dev[i] : store->d_ones.get());
   }
   for (uint32_t j = 0; j < C; ++j) {
      tables[R + j] = reinterpret_cast<uint64_t>(col_filters_dev[j] != nullptr ? col_filters_dev[j] : store->d_ones.get());
   }
   if (tables.size() * sizeof(uint64_t) > SILO_GPU_FILTERS_CROSS_SCRATCH_BYTES(n_rows, n_cols)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_filters_cross: scratch layout exceeds its documented size");  // (cannot happen)
   }
   HIP_TRY(hipSetDevice(store->device));
   auto hip_stream = static_cast<hipStream_t>(stream);
   auto* d_tables = static_cast<uint64_t*>(scratch_dev);
   HIP_TRY(hipMemcpyAsync(d_tables, tables.data(), tables.size() * sizeof(uint64_t), hipMemcpyHostToDevice, hip_stream));
   HIP_TRY(hipStreamSynchronize(hip_stream));  // `tables` is pageable host memory that leaves with this call

   CrossArgs args{};
   args.base = base_filter_dev;
   args.rows = reinterpret_cast<const uint64_t* const*>(d_tables);
   args.cols = args.rows + R;
   args.row_index = reinterpret_cast<const uint32_t*>(d_tables + R + C);
   args.col_index = args.row_index + R;
   args.out = out_dev;
   args.n_rows = R;
   args.n_cols = C;
   args.out_cols = out_cols;
   args.row_words = store->row_words;
   args.sequence_count = store->sequence_count;
   const dim3 grid((store->row_words + CROSS_CHUNK_WORDS - 1) / CROSS_CHUNK_WORDS, (R + CROSS_TILE - 1) / CROSS_TILE, (C + CROSS_TILE - 1) / CROSS_TILE);
   k_cross_filter_counts<<<grid, CROSS_THREADS, 0, hip_stream>>>(args);
   HIP_TRY(hipGetLastError());
   return SILO_GPU_OK;
}

}  // extern "C"
