// silo_gpu_store.hip — a store's lifetime and the order of its stages: create / destroy, the two-pass build (silo_gpu_store_build_pass)
// and finalize, which runs the stages of silo_gpu_store_streams.hip and silo_gpu_store_layout.hip.  The rows come in through
// silo_gpu_store_build.hip.  DESIGN.md sections 2 and 3.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "store_internal.h"

using namespace silo_gpu_detail;

namespace {

__global__ void k_fill_ones(uint64_t* out, uint32_t row_words, uint32_t sequence_count) {
   const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
   if (w < row_words) {
      out[w] = silo_gpu::valid_mask(w, sequence_count);
   }
}

}  // namespace

namespace silo_gpu_detail {

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
int ensureDevice(int device) {
   int count = 0;
   hipError_t err = hipGetDeviceCount(&count);
   if (err != hipSuccess || count == 0) {
      return fail(
         SILO_GPU_ERR_NO_DEVICE,
         "no HIP device visible (hipGetDeviceCount: " + std::string(hipGetErrorString(err)) +
            "); the silo_gpu product path has no CPU fallback"
      );
   }
   if (device < 0 || device >= count) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "device ordinal out of range");
   }
   HIP_TRY(hipSetDevice(device));
   return SILO_GPU_OK;
}

int growSparse(SeqStoreHost& seqstore, uint32_t needed) {
   if (needed <= seqstore.sparse_capacity) {
      return SILO_GPU_OK;
   }
   uint32_t capacity = std::max<uint32_t>(1u << 16, seqstore.sparse_capacity);
   while (capacity < needed) {
      capacity *= 2;
   }
   DeviceArray<uint64_t> bigger;
   HIP_TRY(bigger.alloc(capacity));
   if (seqstore.d_sparse.get() != nullptr) {
      HIP_TRY(hipMemcpy(bigger.get(), seqstore.d_sparse.get(), static_cast<size_t>(seqstore.sparse_capacity) * sizeof(uint64_t), hipMemcpyDeviceToDevice));
   }
   seqstore.d_sparse = std::move(bigger);
   seqstore.sparse_capacity = capacity;
   return SILO_GPU_OK;
}

/// The build-time planes of a sequence store, allocated (zeroed) when its first sequences arrive.
int ensureBuildPlanes(silo_gpu_store* store, SeqStoreHost& seqstore) {
   if (seqstore.layout.built) {
      return fail(
         SILO_GPU_ERR_INVALID_ARGUMENT, "the sequence store is finalized: its build-time planes were re-encoded and released, no sequences can be added"
      );
   }
   SeqStoreDev& dev = seqstore.dev;
   if (dev.scan != nullptr || dev.extra != nullptr || dev.build_mode == BUILD_COUNT) {
      return SILO_GPU_OK;  // (the counting pass of a two-pass build writes no plane at all)
   }
   // the encoding pass of a two-pass build writes the valid symbols straight into the adaptive planes: only the extra planes are built
   const size_t scan_bytes = dev.build_mode == BUILD_ENCODE ? 0 : static_cast<size_t>(dev.positions) * dev.n_bits * dev.row_words * sizeof(uint64_t);
   const size_t extra_bytes = dev.runs_at_build != 0 ? 0 : static_cast<size_t>(dev.positions) * dev.n_extra * dev.row_words * sizeof(uint64_t);
   if (scan_bytes > 0) {
      HIP_TRY(seqstore.d_scan.alloc(scan_bytes / sizeof(uint64_t)));
      dev.scan = seqstore.d_scan.get();
      HIP_TRY(hipMemset(dev.scan, 0, scan_bytes));
   }
   if (extra_bytes > 0) {
      HIP_TRY(seqstore.d_extra.alloc(extra_bytes / sizeof(uint64_t)));
      dev.extra = seqstore.d_extra.get();
      HIP_TRY(hipMemset(dev.extra, 0, extra_bytes));
   }
   dev.planes = dev.scan;
   store->device_bytes += scan_bytes + extra_bytes;
   return SILO_GPU_OK;
}

/// The unfiltered totals of a sequence store (seqstore.d_totals), on the host.
int downloadTotals(const SeqStoreHost& seqstore, std::vector<uint32_t>& totals) {
   totals.resize(static_cast<size_t>(seqstore.dev.positions) * seqstore.dev.n_scan);
   HIP_TRY(hipMemcpy(totals.data(), seqstore.d_totals.get(), totals.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   return SILO_GPU_OK;
}

}  // namespace silo_gpu_detail

extern "C" {

int silo_gpu_store_create(const silo_gpu_store_desc* desc, silo_gpu_store** out) {
   if (desc == nullptr || out == nullptr || desc->n_seqstores == 0 || desc->seqstores == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_create: null descriptor");
   }
   *out = nullptr;
   if (int rc = ensureDevice(desc->device); rc != SILO_GPU_OK) {
      return rc;
   }
   {
      // ONE device per process (one process per GPU, as the engine is deployed): the per-thread side streams, the scratch
      // pools and the kernels' shared-memory attributes are set up once, for the device of the first store
      static std::atomic<int> process_device{-1};
      int expected = -1;
      if (!process_device.compare_exchange_strong(expected, desc->device) && expected != desc->device) {
         return fail(
            SILO_GPU_ERR_UNSUPPORTED, "silo_gpu_store_create: this process holds stores on device " + std::to_string(expected) +
                                         " already; one process serves one GPU (start a process per device)"
         );
      }
   }
   auto* store = new (std::nothrow) silo_gpu_store();
   if (store == nullptr) {
      return fail(SILO_GPU_ERR_OUT_OF_MEMORY, "host allocation failed");
   }
   store->device = desc->device;
   store->sequence_count = desc->sequence_count;
   const uint32_t words = (desc->sequence_count + 63u) / 64u;
   store->row_words = std::max(ROW_ALIGN_WORDS, (words + ROW_ALIGN_WORDS - 1) / ROW_ALIGN_WORDS * ROW_ALIGN_WORDS);
   const uint32_t row_words = store->row_words;

   auto cleanup = [&](int code) {
      silo_gpu_store_destroy(store);
      return code;
   };

   store->seqstores.resize(desc->n_seqstores);
   for (uint32_t k = 0; k < desc->n_seqstores; ++k) {
      const silo_gpu_seqstore_desc& in = desc->seqstores[k];
      SeqStoreHost& seqstore = store->seqstores[k];
      if (in.alphabet > SILO_GPU_ALPHABET_AMINO_ACID || in.positions == 0 || in.reference == nullptr) {
         return cleanup(fail(SILO_GPU_ERR_INVALID_ARGUMENT, "invalid sequence store descriptor"));
      }
      seqstore.alphabet = in.alphabet;
      seqstore.reference.assign(in.reference, in.reference + in.positions);
      SeqStoreDev& dev = seqstore.dev;
      dev.positions = in.positions;
      dev.n_symbols = alphabetSize(in.alphabet);
      dev.n_scan = in.n_scan_symbols;
      dev.n_bits = 0;
      while ((1u << dev.n_bits) < dev.n_scan + 1u) {
         ++dev.n_bits;
      }
      dev.n_extra = in.n_extra_symbols;
      dev.row_words = row_words;
      dev.missing_symbol = missingSymbol(in.alphabet);
      for (uint32_t s = 0; s < SILO_GPU_MAX_SYMBOLS; ++s) {
         dev.kind[s] = PLANE_SPARSE;
         dev.index[s] = 0;
      }
      for (uint32_t s = 0; s < in.n_scan_symbols; ++s) {
         if (in.scan_symbols[s] >= dev.n_symbols) {
            return cleanup(fail(SILO_GPU_ERR_INVALID_ARGUMENT, "scan symbol out of range"));
         }
         dev.kind[in.scan_symbols[s]] = PLANE_SCAN;
         dev.index[in.scan_symbols[s]] = static_cast<uint8_t>(s);
      }
      for (uint32_t s = 0; s < in.n_extra_symbols; ++s) {
         if (in.extra_symbols[s] >= dev.n_symbols || dev.kind[in.extra_symbols[s]] != PLANE_SPARSE) {
            return cleanup(fail(SILO_GPU_ERR_INVALID_ARGUMENT, "extra symbol out of range or duplicated"));
         }
         dev.kind[in.extra_symbols[s]] = PLANE_EXTRA;
         dev.index[in.extra_symbols[s]] = static_cast<uint8_t>(s);
      }
      // the planes are allocated when the first sequences arrive (ensureBuildPlanes) and re-encoded at finalize: stores
      // that are filled and finalized one after the other never hold their build-time planes at the same time
      hipError_t err = hipSuccess;
      if (err == hipSuccess) {
         err = seqstore.d_reference.alloc(in.positions);
      }
      if (err == hipSuccess) {
         err = hipMemcpy(seqstore.d_reference.get(), in.reference, in.positions, hipMemcpyHostToDevice);
      }
      if (err == hipSuccess) {
         err = seqstore.d_sparse_count.alloc(1);
      }
      if (err == hipSuccess) {
         err = hipMemset(seqstore.d_sparse_count.get(), 0, sizeof(uint32_t));
      }
      if (err != hipSuccess) {
         return cleanup(failHip("allocating planes", err));
      }
   }
   hipError_t err = store->d_ones.alloc(row_words);
   if (err == hipSuccess) {
      err = store->d_error_flag.alloc(1);
   }
   if (err == hipSuccess) {
      err = hipMemset(store->d_error_flag.get(), 0, sizeof(uint32_t));
   }
   if (err != hipSuccess) {
      return cleanup(fail(SILO_GPU_ERR_HIP, std::string("allocating store: ") + hipGetErrorString(err)));
   }
   k_fill_ones<<<(row_words + 255) / 256, 256>>>(store->d_ones.get(), row_words, store->sequence_count);
   err = hipDeviceSynchronize();
   if (err != hipSuccess) {
      return cleanup(fail(SILO_GPU_ERR_HIP, std::string("k_fill_ones: ") + hipGetErrorString(err)));
   }
   *out = store;
   return SILO_GPU_OK;
}

void silo_gpu_store_destroy(silo_gpu_store* store) {
   if (store == nullptr) {
      return;
   }
   (void)hipSetDevice(store->device);
   delete store;  // frees what the store and its sequence stores own through DeviceArray members, an unfinished two-pass build (SeqStoreHost::work) included
}

int silo_gpu_store_set_options(silo_gpu_store* store, const silo_gpu_store_options* options) {
   if (store == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_set_options: null store");
   }
   std::lock_guard<std::mutex> lock(store->mutex);
   store->options = options != nullptr ? *options
                                       : silo_gpu_store_options{SILO_GPU_OPTION_DEFAULT, SILO_GPU_OPTION_DEFAULT, SILO_GPU_OPTION_DEFAULT, SILO_GPU_OPTION_DEFAULT};
   return SILO_GPU_OK;
}

uint32_t silo_gpu_store_sequence_count(const silo_gpu_store* store) {
   return store != nullptr ? store->sequence_count : 0;
}
uint32_t silo_gpu_store_row_words(const silo_gpu_store* store) {
   return store != nullptr ? store->row_words : 0;
}
int silo_gpu_store_memory_info(const silo_gpu_store* store, uint64_t* free_bytes, uint64_t* total_bytes) {
   if (store == nullptr || free_bytes == nullptr || total_bytes == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_memory_info: null argument");
   }
   HIP_TRY(hipSetDevice(store->device));
   size_t free_now = 0, total = 0;
   HIP_TRY(hipMemGetInfo(&free_now, &total));
   *free_bytes = free_now;
   *total_bytes = total;
   return SILO_GPU_OK;
}

uint64_t silo_gpu_store_device_bytes(const silo_gpu_store* store) {
   return store != nullptr ? store->device_bytes : 0;
}

namespace {
/// Sorts the sparse keys of one sequence store, re-encodes its build-time planes into the adaptive code planes and derives what
/// the scan reads beside them: the stages of finalize, in their order.
int finalizeSeqStore(silo_gpu_store* store, SeqStoreHost& seqstore) {
   if (seqstore.layout.built) {
      return SILO_GPU_OK;
   }
   if (seqstore.dev.build_mode == BUILD_COUNT) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "the sequence store is in the counting pass of a two-pass build: the encoding pass has to follow before finalize");
   }
   if (const int rc = ensureBuildPlanes(store, seqstore); rc != SILO_GPU_OK) {  // a store that never received a sequence: all-zero planes
      return rc;
   }
   uint32_t count = 0;
   HIP_TRY(hipMemcpy(&count, seqstore.d_sparse_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost));
   count = std::min(count, seqstore.sparse_capacity);
   seqstore.sparse_sorted.resize(count);
   if (count > 0) {
      HIP_TRY(hipMemcpy(seqstore.sparse_sorted.data(), seqstore.d_sparse.get(), static_cast<size_t>(count) * sizeof(uint64_t), hipMemcpyDeviceToHost));
      std::sort(seqstore.sparse_sorted.begin(), seqstore.sparse_sorted.end());
      // a replayed batch may have appended duplicates
      seqstore.sparse_sorted.erase(std::unique(seqstore.sparse_sorted.begin(), seqstore.sparse_sorted.end()), seqstore.sparse_sorted.end());
      count = static_cast<uint32_t>(seqstore.sparse_sorted.size());
      HIP_TRY(hipMemcpy(seqstore.d_sparse.get(), seqstore.sparse_sorted.data(), static_cast<size_t>(count) * sizeof(uint64_t), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(seqstore.d_sparse_count.get(), &count, sizeof(uint32_t), hipMemcpyHostToDevice));
   }
   seqstore.finalized = true;
   // the missing symbol first: its plane goes before the adaptive planes come (a lower peak), and only a store that keeps it as
   // runs may derive the most numerous symbol of a position (planLayout)
   if (const int rc = compactMissingPlane(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = buildLayout(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = buildRunSliceIndex(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = buildGapEvents(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = buildPruneBounds(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   if (const int rc = buildRowBounds(store, seqstore); rc != SILO_GPU_OK) {
      return rc;
   }
   return buildEndRuns(store, seqstore);
}
}  // namespace

int silo_gpu_store_build_pass(silo_gpu_store* store, uint32_t seqstore_id, int pass) {
   if (store == nullptr || seqstore_id >= store->seqstores.size() || (pass != 1 && pass != 2)) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_build_pass: bad arguments (pass 1 = counting, 2 = encoding)");
   }
   std::lock_guard<std::mutex> lock(store->mutex);
   HIP_TRY(hipSetDevice(store->device));
   SeqStoreHost& seqstore = store->seqstores[seqstore_id];
   SeqStoreDev& dev = seqstore.dev;
   if (seqstore.layout.built) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_build_pass: the sequence store is finalized");
   }
   const size_t n_counters = static_cast<size_t>(dev.positions) * dev.n_scan;
   if (pass == 1) {
      if (dev.scan != nullptr || dev.extra != nullptr || dev.build_mode != BUILD_PLANES) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_build_pass: the counting pass has to come before any sequence of the store");
      }
      if (seqstore.d_totals.get() == nullptr) {
         HIP_TRY(seqstore.d_totals.alloc(std::max<size_t>(n_counters, 1)));
      }
      HIP_TRY(hipMemset(seqstore.d_totals.get(), 0, std::max<size_t>(n_counters, 1) * sizeof(uint32_t)));
      HIP_TRY(hipStreamSynchronize(nullptr));
      seqstore.totals_ready = false;
      dev.enc_counts = seqstore.d_totals.get();
      dev.build_mode = BUILD_COUNT;
      // the missing symbol, where it is the store's only extra plane, is counted (and then written) as runs right away
      dev.runs_at_build = dev.n_extra == 1 && dev.kind[dev.missing_symbol] == PLANE_EXTRA && dev.index[dev.missing_symbol] == 0 && missingRunsOption(store) >= 0 ? 1 : 0;
      if (dev.runs_at_build != 0) {
         if (seqstore.d_run_count.get() == nullptr) {
            HIP_TRY(seqstore.d_run_count.alloc(1));
         }
         HIP_TRY(hipMemset(seqstore.d_run_count.get(), 0, sizeof(unsigned long long)));
         HIP_TRY(hipStreamSynchronize(nullptr));
         dev.enc_run_count = seqstore.d_run_count.get();
      }
      return SILO_GPU_OK;
   }
   if (dev.build_mode != BUILD_COUNT) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_build_pass: the encoding pass follows the counting pass");
   }
   HIP_TRY(hipDeviceSynchronize());  // every count of the first pass has landed
   {  // the sparsely stored symbols the first pass counted (it stored none): room for all of them, the counter starts over
      uint32_t counted = 0;
      HIP_TRY(hipMemcpy(&counted, seqstore.d_sparse_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost));
      if (counted > 0xFFFF0000u) {
         return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "two-pass build: too many sparsely stored symbols");
      }
      if (const int rc = growSparse(seqstore, counted + 1u); rc != SILO_GPU_OK) {
         return rc;
      }
      const uint32_t zero = 0;
      HIP_TRY(hipMemcpy(seqstore.d_sparse_count.get(), &zero, sizeof(uint32_t), hipMemcpyHostToDevice));
   }
   dev.build_mode = BUILD_PLANES;
   dev.enc_counts = nullptr;
   seqstore.totals_ready = true;
   const bool runs_counted = dev.runs_at_build != 0;
   dev.runs_at_build = 0;
   if (!reencodes(store, dev)) {
      seqstore.totals_ready = false;
      return SILO_GPU_OK;  // a store that keeps its identity planes: the second pass builds them the ordinary way
   }
   auto work = std::make_shared<SeqStoreHost::LayoutWork>();
   bool fits = false;
   unsigned long long n_runs = 0;
   if (runs_counted) {
      HIP_TRY(hipMemcpy(&n_runs, seqstore.d_run_count.get(), sizeof(n_runs), hipMemcpyDeviceToHost));
   }
   // (the most numerous symbol of a position is derived only where the missing symbol is kept as runs)
   if (const int rc = planLayout(store, seqstore, *work, true, runs_counted && n_runs < (1ull << 32) && seqstore.rows_filled == store->sequence_count, &fits); rc != SILO_GPU_OK) {
      return rc;
   }
   if (!fits) {
      seqstore.totals_ready = false;
      return SILO_GPU_OK;
   }
   if (runs_counted) {  // the runs of the missing symbol: exactly as many slots as the first pass counted
      if (n_runs < (1ull << 32)) {
         const size_t slots = std::max<size_t>(n_runs, 1);
         HIP_TRY(seqstore.d_missing_run_keys.alloc(slots));
         HIP_TRY(seqstore.d_missing_run_ends.alloc(slots));
         HIP_TRY(hipMemset(seqstore.d_run_count.get(), 0, sizeof(unsigned long long)));
         HIP_TRY(hipStreamSynchronize(nullptr));
         dev.enc_run_keys = seqstore.d_missing_run_keys.get();
         dev.enc_run_ends = seqstore.d_missing_run_ends.get();
         dev.enc_run_capacity = n_runs;
         dev.runs_at_build = 1;
      }
   }
   dev.enc_code_map = work->d_code_map.get();
   dev.enc_row_of = work->d_row_of.get();
   dev.enc_planes = work->d_planes.get();
   dev.enc_first = work->d_first.get();
   dev.enc_cursor = work->d_cursor.get();
   dev.enc_escapes = work->d_escapes.get();
   dev.build_mode = BUILD_ENCODE;
   seqstore.work = std::move(work);
   return SILO_GPU_OK;
}

int silo_gpu_store_build_mode(const silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size()) {
      return -1;
   }
   return static_cast<int>(store->seqstores[seqstore_id].dev.build_mode);
}

int silo_gpu_store_finalize(silo_gpu_store* store) {
   if (store == nullptr) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_finalize: null store");
   }
   std::lock_guard<std::mutex> lock(store->mutex);
   HIP_TRY(hipSetDevice(store->device));
   for (SeqStoreHost& seqstore : store->seqstores) {
      if (const int rc = finalizeSeqStore(store, seqstore); rc != SILO_GPU_OK) {
         return rc;
      }
   }
   return SILO_GPU_OK;
}

int silo_gpu_store_finalize_seqstore(silo_gpu_store* store, uint32_t seqstore_id) {
   if (store == nullptr || seqstore_id >= store->seqstores.size()) {
      return fail(SILO_GPU_ERR_INVALID_ARGUMENT, "silo_gpu_store_finalize_seqstore: bad arguments");
   }
   std::lock_guard<std::mutex> lock(store->mutex);
   HIP_TRY(hipSetDevice(store->device));
   return finalizeSeqStore(store, store->seqstores[seqstore_id]);
}


}  // extern "C"
