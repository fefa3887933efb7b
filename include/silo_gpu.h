/*
 * silo_gpu.h — C ABI of the MI355X (gfx950) device side of the SILO mutation-filter hot path.
 *
 * This is the drop-in boundary described in SURVEY.md §8(b): plain pointers and sizes, no C++/torch
 * types, 0 on success / negative silo_gpu_status on failure, never throws.  The reference has no FFI
 * layer; each entry point below names the reference C++ interface (file:line under the reference
 * tree) whose arithmetic it replaces.
 *
 * Data model: a *store* is one DatabasePartition (database_partition.h:39-112) with
 * `sequence_count` rows.  Every sequence store in it (nucleotide segment or gene) is a
 * SequenceStorePartition (sequence_store.h:34-88) restated as dense bitsets in HBM:
 *   row_words  Wp = roundup(ceil(N/64), 32)   (256-byte aligned rows, tail bits zero)
 *   scan planes   [position][valid mutation symbol][Wp]   uint64, bit i of word w = sequence 64*w+i
 *   extra planes  [extra dense symbol][position][Wp]      (the missing symbol N / X, ...)
 *   sparse symbols (IUPAC ambiguity codes) as sorted (position, symbol, sequence id) triples.
 */
#ifndef SILO_GPU_H
#define SILO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
   SILO_GPU_OK = 0,
   SILO_GPU_ERR_INVALID_ARGUMENT = -1,
   SILO_GPU_ERR_OUT_OF_MEMORY = -2,
   SILO_GPU_ERR_HIP = -3,         /* a HIP runtime call failed; see silo_gpu_last_error() */
   SILO_GPU_ERR_NO_DEVICE = -4,   /* no gfx950 device visible: the product path has no CPU fallback */
   SILO_GPU_ERR_PROGRAM_TOO_LARGE = -5,
   SILO_GPU_ERR_UNSUPPORTED = -6
} silo_gpu_status;

/* Alphabets.  Symbol ids are the reference enum values:
 * nucleotide_symbols.h:15-32 (GAP A C G T R Y S W K M B D H V N = 0..15),
 * aa_symbols.h:15-41 (GAP A C D E F G H I K L M N P Q R S T V W Y B Z STOP X = 0..24). */
enum { SILO_GPU_ALPHABET_NUCLEOTIDE = 0, SILO_GPU_ALPHABET_AMINO_ACID = 1 };
enum { SILO_GPU_NUC_SYMBOLS = 16, SILO_GPU_AA_SYMBOLS = 25, SILO_GPU_MAX_SYMBOLS = 25 };
#define SILO_GPU_SYMBOL_NONE 0xFFu

typedef struct silo_gpu_store silo_gpu_store; /* opaque; one per device shard */

/* One SequenceStorePartition (sequence_store.h:51-56). */
typedef struct {
   uint32_t alphabet;         /* SILO_GPU_ALPHABET_* */
   uint32_t positions;        /* reference_sequence.size() */
   const uint8_t* reference;  /* [positions] symbol ids (reference_genomes.cpp) */
   /* Dense planes to allocate.  scan_symbols must be the alphabet's VALID_MUTATION_SYMBOLS in
    * their declared order (nucleotide_symbols.h:61-67, aa_symbols.h:56-79): they form the
    * [position][symbol] block the Mutations scan streams.  extra_symbols are further dense planes
    * (normally the missing symbol, SYMBOL_MISSING).  Symbols in neither list are kept sparse. */
   uint32_t n_scan_symbols;
   const uint8_t* scan_symbols;
   uint32_t n_extra_symbols;
   const uint8_t* extra_symbols;
} silo_gpu_seqstore_desc;

typedef struct {
   int32_t device;            /* HIP device ordinal */
   uint32_t sequence_count;   /* DatabasePartition::sequence_count (capacity; rows are 0..N-1) */
   uint32_t n_seqstores;
   const silo_gpu_seqstore_desc* seqstores;
} silo_gpu_store_desc;

/* How finalize lays a store out — per STORE (two engines of one process may differ); a field left at SILO_GPU_OPTION_DEFAULT
 * follows the process-wide silo_gpu_tune knob of the same meaning (those are for probes and tests).  Set before finalize. */
#define SILO_GPU_OPTION_DEFAULT INT32_MIN
typedef struct silo_gpu_store_options {
   int32_t layout;           /* as SILO_GPU_TUNE_COMPACT_INDEX: < 0 keep the build-time identity planes, 0 re-encode every position into its
                                cheapest layout (the most numerous symbol derived where the missing symbol is kept as runs), 2 without one-hot
                                rows, 3 with a one-hot row for the most numerous symbol too */
   int32_t missing_runs;     /* as SILO_GPU_TUNE_MISSING_RUNS: < 0 keeps the plane of the missing symbol */
   int32_t key_cost;         /* as SILO_GPU_TUNE_KEY_COST: > 0 = plane bytes an escape key costs in the choice of layouts */
   int32_t launch_cost_kib;  /* as SILO_GPU_TUNE_LAUNCH_COST */
} silo_gpu_store_options;

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Allocates zeroed planes in HBM.  Replaces SequenceStorePartition's constructor
 * (sequence_store.cpp:21-29).  Fails with SILO_GPU_ERR_NO_DEVICE when no GPU is present, and with SILO_GPU_ERR_UNSUPPORTED for a
 * device other than that of the process's first store: one process serves one GPU. */
int silo_gpu_store_create(const silo_gpu_store_desc* desc, silo_gpu_store** out);
void silo_gpu_store_destroy(silo_gpu_store* store);

/* NULL resets every field to SILO_GPU_OPTION_DEFAULT.  Stores that are finalized already keep their layout. */
int silo_gpu_store_set_options(silo_gpu_store* store, const silo_gpu_store_options* options);

uint32_t silo_gpu_store_sequence_count(const silo_gpu_store* store);
uint32_t silo_gpu_store_row_words(const silo_gpu_store* store); /* Wp, in uint64 words */
uint64_t silo_gpu_store_device_bytes(const silo_gpu_store* store);
/* Free and total memory of the store's device (hipMemGetInfo), for callers that choose between the one-pass and the two-pass build. */
int silo_gpu_store_memory_info(const silo_gpu_store* store, uint64_t* free_bytes, uint64_t* total_bytes);

/* ---- index build: SequenceStorePartition::fill / interpret (sequence_store.cpp:31-66,100-220) - */

/* Transposes a batch of aligned sequences into the planes on the device.
 * `chars` is host memory, row-major [n_sequences][positions], the characters of the alignment
 * (charToSymbol: nucleotide_symbols.cpp:46-85, aa_symbols.cpp:62-117).  `is_null[i] != 0` marks a
 * missing genome: the missing symbol at every position (sequence_store.cpp:166-169); its chars are
 * ignored.  is_null may be NULL.  first_sequence + n_sequences <= sequence_count.
 * An illegal character fails with SILO_GPU_ERR_INVALID_ARGUMENT (sequence_store.cpp:118-122). */
int silo_gpu_store_append_sequences(
   silo_gpu_store* store, uint32_t seqstore_id, uint32_t first_sequence, uint32_t n_sequences,
   const char* chars, const uint8_t* is_null
);

/* ---- import from the reference's own storage form (the roaring payloads of a snapshot) ---------------
 * A reference Position (position.h:27-37) is one roaring bitmap per symbol — written by saveDatabaseState in CRoaring's
 * portable serialization (roaring_serialize.h:17-45) — with the most numerous symbol stored FLIPPED (its complement) or
 * DELETED (empty; position.cpp:42-127), and the missing symbol kept ROW-wise (missing_symbol_bitmaps[row] = the positions
 * where the row has N / X, sequence_store.cpp:153-190).  silo_gpu_store_import_missing_rows first (the deleted symbol of a
 * position is "no other symbol and not missing"), then silo_gpu_store_import_position per position; finalize as usual.
 * The containers are expanded on the device.  The Boost archive framing around the payloads is the caller's to strip: it is
 * not read here (nothing in this image to pin it against), and the portable format itself is restated from its published
 * specification — parity unpinned.  SILO_GPU_SYMBOL_NONE = no flipped / deleted symbol.
 * Two rules of silo_gpu_store_import_position, both refused with SILO_GPU_ERR_INVALID_ARGUMENT:
 *   - a position takes ONE import.  A row has one symbol at a position: bitmaps of one call that share a row are refused, and so
 *     is any further call for a position whose planes an earlier call has written, whatever symbols it names (scan symbols,
 *     sparsely stored ambiguity codes and extra-plane symbols alike).  A call refused for its arguments or for a malformed first
 *     payload has written nothing and may be repeated; after any other refusal the position's content is undefined.
 *   - the flipped symbol's bitmap has to be among the payloads, EMPTY included: flipped, an empty bitmap stands for every row.
 *     A flipped_symbol without a payload is refused rather than read as "no row" (the deleted symbol, by contrast, needs none).
 * Ids at or past sequence_count inside a payload (positions at or past the store's, for the missing rows) are ignored. */
typedef struct silo_gpu_roaring_payload {
   uint32_t symbol;    /* reference enum value; ignored by silo_gpu_store_import_missing_rows */
   const void* bytes;  /* portable-format roaring bitmap, host memory */
   size_t n_bytes;
} silo_gpu_roaring_payload;
int silo_gpu_store_import_missing_rows(
   silo_gpu_store* store, uint32_t seqstore_id, uint32_t first_sequence, uint32_t n_sequences, const silo_gpu_roaring_payload* rows
);
int silo_gpu_store_import_position(
   silo_gpu_store* store, uint32_t seqstore_id, uint32_t position, const silo_gpu_roaring_payload* bitmaps, uint32_t n_bitmaps,
   uint32_t flipped_symbol, uint32_t deleted_symbol
);

/* Two-pass build of a sequence store — for stores too large to hold their build-time planes beside the finished ones (the
 * build-time planes are 3 / 5 per position; a finished nucleotide store about one): stream the sequences TWICE.
 *   silo_gpu_store_build_pass(store, id, 1)   before the first sequence: the appends / generate calls that follow only COUNT
 *                                             the valid symbols per position (no plane is allocated);
 *   silo_gpu_store_build_pass(store, id, 2)   after all sequences have been seen once: the layout of every position is chosen
 *                                             from the counts, the adaptive planes are allocated, and the same appends /
 *                                             generate calls, repeated, write every row straight into them;
 *   silo_gpu_store_finalize / _finalize_seqstore as usual (the escape keys are sorted; the missing symbol becomes runs).
 * A store that would keep its identity planes anyway (short rows, compact_scan_index off) simply builds them in the second
 * pass.  silo_gpu_store_build_mode: 0 ordinary, 1 counting, 2 encoding.  The roaring import is not available in this mode. */
int silo_gpu_store_build_pass(silo_gpu_store* store, uint32_t seqstore_id, int pass);
int silo_gpu_store_build_mode(const silo_gpu_store* store, uint32_t seqstore_id);

/* Sorts the sparse triples gathered by append/generate; call once after the last append and
 * before any query.  (The reference's optimizeBitmaps, sequence_store.cpp:192-211, has no dense
 * analogue: flipped/deleted bitmaps are storage tricks) */
int silo_gpu_store_finalize(silo_gpu_store* store);

/* Synthetic SARS-CoV-2-shaped data written straight into the planes (bench / parity tests only;
 * the model is specified in DESIGN.md §6 and restated on the CPU in oracle/synth.py).
 * All arrays are host memory.  lineage_symbol is [positions][n_lineages], 0xFF = "reference". */
typedef struct {
   uint64_t seed;
   uint32_t n_lineages;
   const uint16_t* lineage_of_sequence; /* [N] */
   const uint32_t* lead_gap;            /* [N] positions [0, lead_gap) are GAP */
   const uint32_t* trail_gap;           /* [N] positions [P - trail_gap, P) are GAP */
   const uint32_t* missing_start;       /* [N] run of the missing symbol */
   const uint32_t* missing_len;         /* [N] */
   const uint8_t* lineage_symbol;       /* [positions][n_lineages] */
   uint32_t private_threshold;          /* of 2^20: P(private substitution) per cell */
   uint32_t ambiguous_threshold;        /* of 2^24: P(sparse ambiguity code) per cell */
   /* Position-range shards: the store holds positions [position_offset, position_offset + positions)
    * of a genome of total_positions (0 = the store's own length); lineage_symbol covers the slice. */
   uint32_t position_offset;
   uint32_t total_positions;
} silo_gpu_synth_desc;
int silo_gpu_store_generate_synthetic(
   silo_gpu_store* store, uint32_t seqstore_id, const silo_gpu_synth_desc* synth
);

/* ---- device buffers owned by the caller -------------------------------------------------------- */

/* Row-sized (Wp words) bitset in HBM, zero-initialised.  Used for filter results and for host-built
 * metadata bitsets (pango lineage sets: pango_lineage_column.cpp:57-77, uploaded once). */
int silo_gpu_bitset_alloc(const silo_gpu_store* store, uint64_t** out_dev);
int silo_gpu_bitset_upload(const silo_gpu_store* store, uint64_t* dst_dev, const uint64_t* src_host, size_t n_words, void* stream);
int silo_gpu_bitset_download(const silo_gpu_store* store, uint64_t* dst_host, const uint64_t* src_dev, size_t n_words, void* stream);
/* bit i = membership_by_lineage[lineage_of_sequence[i]] for a store filled by generate_synthetic. */
int silo_gpu_bitset_from_lineages(const silo_gpu_store* store, uint64_t* dst_dev, const uint8_t* membership_by_lineage, uint32_t n_lineages, void* stream);
/* Dictionary-encoded metadata column kept on the device: bit i = membership_by_value[value_ids_dev[i]].
 * This is how a metadata predicate (pango lineage, pango_lineage_filter.cpp:37-59) enters the device path. */
int silo_gpu_upload_u32(const uint32_t* src_host, size_t n, uint32_t** out_dev);
int silo_gpu_bitset_from_value_ids(const silo_gpu_store* store, uint64_t* dst_dev, const uint32_t* value_ids_dev, const uint8_t* membership_by_value, uint32_t n_values, void* stream);
void silo_gpu_free(void* dev_ptr);
int silo_gpu_malloc(size_t bytes, void** out_dev);
int silo_gpu_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream); /* synchronises */
int silo_gpu_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream); /* synchronises */
/* Result tables fetched without stalling the stream: page-locked host memory + a copy that is only enqueued
 * (wait for it with an event recorded after it, silo_gpu_event_synchronize).  The host mirror fetches the
 * counts[P][S] table of sequence store k while the scans of stores k+1.. are still running. */
int silo_gpu_host_alloc(size_t bytes, void** out_host);
void silo_gpu_host_free(void* host);
int silo_gpu_memcpy_d2h_async(void* dst_pinned_host, const void* src_dev, size_t bytes, void* stream);
int silo_gpu_stream_synchronize(void* stream);
/* A non-blocking HIP stream (does not synchronise with the null stream); every `void* stream` parameter of
 * this ABI accepts one, or NULL for the null stream. */
int silo_gpu_stream_create(void** out_stream);
/* Selects the HIP device of the CALLING host thread (HIP keeps the current device per thread, starting at 0): a thread that
 * creates streams, events or buffers for a store on device r selects r first.  Entry points that take a store select its
 * device themselves. */
int silo_gpu_set_device(int device);
void silo_gpu_stream_destroy(void* stream);

/* Device pointer of the one-hot plane of (seqstore, position, symbol) when the store holds one: the extra symbols
 * (the missing symbol N / X).  NULL for the valid mutation symbols — they live in the bit-sliced scan planes
 * ([position][code bit][Wp], code = index among the scan symbols + 1; 3 planes for 5 nucleotide symbols, 5 for 22
 * amino-acid symbols) — and for sparsely stored symbols; silo_gpu_store_sparse_plane materialises either.
 * Replaces SequenceStorePartition::getBitmap (sequence_store.cpp:92-98); positions are 0-based as there. */
const uint64_t* silo_gpu_store_plane(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t position, uint32_t symbol);

/* Materialises the one-hot bitset of any symbol at a position into dst_dev (Wp words, overwritten): decoded from the
 * code planes (valid mutation symbols), copied (extra symbols) or scattered from the sorted keys (sparse symbols). */
int silo_gpu_store_sparse_plane(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t position, uint32_t symbol, uint64_t* dst_dev, void* stream);

/* ---- K3: fused filter-expression evaluator --------------------------------------------------------
 * Replaces Operator::evaluate() of IndexScan / Complement / Intersection / Union / Threshold /
 * Full / Empty / BitmapSelection (operators/index_scan.cpp:28-30, complement.cpp:50-54,
 * intersection.cpp:62-127, union.cpp:35-45, threshold.cpp:64-138, full.cpp:24-28, empty.cpp,
 * bitmap_selection.cpp:33-52): the whole operator tree of one partition is one launch.
 *
 * A bit-program is a register machine over 64-bit slots, one program run per bitset word.
 * Instruction word 0: op | dst<<8 | a<<16 | b<<24, word 1: imm.   Slot 0 holds the result. */
enum {
   SILO_GPU_OP_LOAD = 0,     /* dst = leaves[imm][w]                                  (IndexScan) */
   SILO_GPU_OP_ZERO = 1,     /* dst = 0                                               (Empty)     */
   SILO_GPU_OP_ONES = 2,     /* dst = valid(w): all rows < sequence_count             (Full)      */
   SILO_GPU_OP_NOT = 3,      /* dst = ~a & valid(w)                                   (Complement)*/
   SILO_GPU_OP_AND = 4,      /* dst = a & b                                           (Intersection) */
   SILO_GPU_OP_OR = 5,       /* dst = a | b                                           (Union)     */
   SILO_GPU_OP_ANDNOT = 6,   /* dst = a & ~b                                          (Intersection, negated child) */
   SILO_GPU_OP_CNT_ADD = 7,  /* bit-sliced counter in slots dst..dst+b-1 += slot a    (Threshold) */
   SILO_GPU_OP_CNT_GE = 8,   /* dst = (counter in slots a..a+b-1) >= imm                           */
   SILO_GPU_OP_CNT_EQ = 9,   /* dst = (counter in slots a..a+b-1) == imm                           */
   SILO_GPU_OP_MOV = 10,     /* dst = a */
   /* n-ary forms over a run of consecutive leaves, imm = first_leaf | count << 16 (count >= 1): the leaves
    * are fetched 8 at a time with independent loads (flat Or / And / N-Of over stored columns). */
   SILO_GPU_OP_OR_N = 11,          /* dst = leaf[first] | ... | leaf[first+count-1]          (Union)        */
   SILO_GPU_OP_AND_N = 12,         /* dst = leaf[first] & ... & leaf[first+count-1]          (Intersection) */
   SILO_GPU_OP_CNT_ADD_N = 13,     /* counter dst..dst+b-1 += each leaf of the run           (Threshold)    */
   SILO_GPU_OP_CNT_ADD_NOT_N = 14  /* counter dst..dst+b-1 += each (~leaf & valid) of the run (negated children) */
};
enum { SILO_GPU_MAX_INSTRUCTIONS = 320, SILO_GPU_MAX_LEAVES = 128, SILO_GPU_MAX_SLOTS = 32 };
/* A source operand (a, b) >= SILO_GPU_LEAF_OPERAND reads leaf (operand - SILO_GPU_LEAF_OPERAND) directly, so a
 * leaf needs no LOAD instruction of its own; destinations are always slots. */
enum { SILO_GPU_LEAF_OPERAND = 32 };
/* Cardinalities are accumulated into SILO_GPU_COUNT_SHARDS consecutive uint64 counters (to keep device
 * atomics off a single word); the total is their sum.  Buffers passed as out_count_dev have that many. */
enum { SILO_GPU_COUNT_SHARDS = 64 };

typedef struct {
   uint32_t n_instructions;
   const uint32_t* code;            /* 2 * n_instructions words, host memory */
   uint32_t n_leaves;
   const uint64_t* const* leaves;   /* device pointers, each Wp words, host array */
   uint32_t n_slots;                /* slots used, <= SILO_GPU_MAX_SLOTS */
} silo_gpu_bitprog;

/* out_bitset_dev (Wp words) and/or out_count_dev (SILO_GPU_COUNT_SHARDS uint64, ACCUMULATED into, so the
 * caller can sum partitions like aggregated.cpp:58-66) may be NULL. */
int silo_gpu_filter_eval(
   const silo_gpu_store* store, const silo_gpu_bitprog* program,
   uint64_t* out_bitset_dev, uint64_t* out_count_dev, void* stream
);

/* K3 for a batch of programs over one store in ONE launch: the filter -> Aggregated queries that are in flight at the
 * same time (the reference evaluates each on its own request thread: intersection.cpp:111-126, union.cpp:39-44,
 * threshold.cpp:93-128 once per request).  A single 32-column program is launch-latency bound (40 MB at 10 M
 * sequences); a batch streams at memory speed.  out_bitsets_dev (may be NULL, entries may be NULL): per program a
 * row-sized device bitset to receive the result; out_counts (host memory, may be NULL): the cardinalities.
 * Synchronises `stream` before it returns.  Programs obey the limits of silo_gpu_filter_eval. */
int silo_gpu_filter_eval_batch(
   const silo_gpu_store* store, const silo_gpu_bitprog* programs, uint32_t n_programs, uint64_t* const* out_bitsets_dev, uint64_t* out_counts,
   void* stream
);

/* ---- K2: cardinality (aggregated.cpp:61, mutations.cpp:45) ---------------------------------------- */
/* Count slot: the cardinality of a filter without a copy, a device-side reduction or a stream synchronisation.  Every block
 * of the K3 launch stores the rows IT selected into page-locked host memory (one posted 8-byte system-scope store, tagged
 * with the launch's epoch); silo_gpu_count_slot_wait spins on those words and adds them up (after a spin budget of tens of
 * milliseconds it synchronises the stream once, so a failed launch is an error, not a hang).  One slot serves one launch at
 * a time; a host thread keeps its own.  Replaces roaring::cardinality() at the end of Operator::evaluate for Aggregated
 * (aggregated.cpp:61). */
typedef struct silo_gpu_count_slot silo_gpu_count_slot;
int silo_gpu_count_slot_create(silo_gpu_count_slot** out_slot);
void silo_gpu_count_slot_destroy(silo_gpu_count_slot* slot);
int silo_gpu_filter_eval_count(
   const silo_gpu_store* store, const silo_gpu_bitprog* program, uint64_t* out_bitset_dev /* may be NULL */, silo_gpu_count_slot* slot,
   void* stream
);
int silo_gpu_count_slot_wait(silo_gpu_count_slot* slot, uint64_t* out_count, void* stream);
int silo_gpu_popcount(const silo_gpu_store* store, const uint64_t* bitset_dev, uint64_t* out_count_dev /* shards, accumulated */, void* stream);

/* ---- K5 / K6: metadata columns -------------------------------------------------
 * A column is a plain device array with one value per row: int32 (int columns, NULL = INT32_MIN), uint32 (dates as
 * year<<16|month<<12|day, NULL = 0; dictionary ids of string / lineage columns) or double (NULL = NaN).
 * silo_gpu_bitset_from_compare evaluates one predicate of the reference's Selection operator for all rows:
 * bit i = values[i] <comparator> *value with the C++ comparison operators (CompareToValueSelection<T>::match,
 * selection.cpp:145-165) — a metadata predicate enters the fused filter program as this bitset. */
#define SILO_GPU_VALUE_I32 0
#define SILO_GPU_VALUE_U32 1
#define SILO_GPU_VALUE_F64 2
#define SILO_GPU_CMP_EQUALS 0
#define SILO_GPU_CMP_NOT_EQUALS 1
#define SILO_GPU_CMP_LESS 2
#define SILO_GPU_CMP_HIGHER_OR_EQUALS 3
#define SILO_GPU_CMP_HIGHER 4
#define SILO_GPU_CMP_LESS_OR_EQUALS 5
int silo_gpu_upload_column(const void* src_host, size_t n_rows, int value_type, void** out_dev); /* free: silo_gpu_free */
int silo_gpu_bitset_from_compare(
   const silo_gpu_store* store, uint64_t* dst_dev, const void* values_dev, int value_type, int comparator,
   const void* value /* one int32 / uint32 / double on the host */, void* stream
);
/* Aggregated with groupByFields (aggregated.cpp:100-149) for columns given as dictionary ids: for every row i of
 * the filter (NULL = all rows) counts_dev[sum_c ids[c][i] * stride_c] += 1 with mixed-radix strides, the first
 * column most significant; prod(cardinalities) <= SILO_GPU_MAX_GROUP_BINS entries, accumulated into (zero them
 * first; partitions with a shared dictionary may share one table). */
#define SILO_GPU_MAX_GROUP_COLUMNS 8
#define SILO_GPU_MAX_GROUP_BINS (1u << 24)
int silo_gpu_group_count(
   const silo_gpu_store* store, const uint64_t* filter_dev, const uint32_t* const* group_ids_dev, const uint32_t* cardinalities,
   uint32_t n_columns, uint32_t* counts_dev, void* stream
);
/* The same group-by for tuple spaces beyond SILO_GPU_MAX_GROUP_BINS (up to 2^64 - 1 potential tuples): a hash table
 * in HBM keyed by the 64-bit mixed-radix tuple id, then compacted.  max_rows bounds the number of selected rows (the
 * filter's cardinality; the table gets twice as many slots).  On success *out_keys_dev / *out_counts_dev hold
 * *out_n_groups (tuple id, count) pairs in no particular order; free both with silo_gpu_free.  Synchronises. */
int silo_gpu_group_count_hashed(
   const silo_gpu_store* store, const uint64_t* filter_dev, const uint32_t* const* group_ids_dev, const uint32_t* cardinalities,
   uint32_t n_columns, uint32_t max_rows, uint64_t** out_keys_dev, uint32_t** out_counts_dev, uint32_t* out_n_groups, void* stream
);
/* Insertion index on the device (insertion_index.cpp, insertions.cpp:186-221).  The occurrences of a column's
 * insertions in one sequence are n_pairs pairs (rows_dev[k], ids_dev[k]): row k carries the distinct insertion
 * ids_dev[k] (< n_ids).  silo_gpu_bitset_from_pairs: dst = rows of the pairs whose insertion is a member
 * (membership_by_id on the host: the distinct insertions the search pattern matched, InsertionContains);
 * silo_gpu_count_pairs: counts_dev[id] += number of pairs of that insertion whose row is in the filter (NULL = all
 * rows), the and_cardinality per insertion of the Insertions action. */
int silo_gpu_bitset_from_pairs(
   const silo_gpu_store* store, uint64_t* dst_dev, const uint32_t* rows_dev, const uint32_t* ids_dev, uint32_t n_pairs,
   const uint8_t* membership_by_id, uint32_t n_ids, void* stream
);
int silo_gpu_count_pairs(
   const silo_gpu_store* store, const uint64_t* filter_dev, const uint32_t* rows_dev, const uint32_t* ids_dev, uint32_t n_pairs,
   uint32_t* counts_dev, void* stream
);
/* FastaAligned (fasta_aligned.cpp:44-83 reconstructSequence): the stored symbol of every position of the given
 * rows as characters, out_chars_dev[r * positions + p]; row_ids_dev holds n_rows sequence ids of this store. */
int silo_gpu_reconstruct_sequences(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint32_t* row_ids_dev, uint32_t n_rows, char* out_chars_dev, void* stream
);

/* ---- K4: row selection of Mutations (mutations.cpp:184-232) ------------------------------------------
 * For every position p < n_positions with total = sum_s counts[p][s] > 0, every symbol index s != reference_index[p]
 * (0xFF = the reference symbol is not a valid mutation symbol) with
 *     counts[p][s] > (min_proportion == 0 ? 0 : (uint32_t)(ceil((double)total * min_proportion) - 1))
 * is appended to the list in out_dev: word 0 = number of selected cells (may exceed `capacity`: then only the
 * first `capacity` appended rows are stored and the caller falls back to the whole table), words 1-3 unused,
 * rows from word 4.  Rows are unordered.  out_dev holds 16 + 16 * capacity bytes. */
typedef struct silo_gpu_mutation_row {
   uint32_t position;     /* 0-based, relative to counts_dev */
   uint32_t symbol_index; /* index into the sequence store's valid mutation symbols */
   uint32_t count;
   uint32_t total;
} silo_gpu_mutation_row;
int silo_gpu_mutations_select(
   const uint32_t* counts_dev, const uint8_t* reference_index_dev, uint32_t n_positions, uint32_t n_symbols, double min_proportion,
   uint32_t capacity, uint32_t* out_dev, void* stream
);
/* K4 with the list delivered straight into page-locked host memory: a row slot owns a host buffer the kernel writes the
 * selected rows into and a header word its last block publishes (no device -> host copy, no event: the host spins on the
 * word as for a count slot).  One slot serves one launch at a time.  *out_selected may exceed the slot's capacity: only the
 * first `capacity` rows are there and the caller falls back to the whole table, as with silo_gpu_mutations_select.
 * The rows stay valid until the slot's next launch. */
typedef struct silo_gpu_row_slot silo_gpu_row_slot;
int silo_gpu_row_slot_create(uint32_t row_capacity, silo_gpu_row_slot** out_slot);
void silo_gpu_row_slot_destroy(silo_gpu_row_slot* slot);
int silo_gpu_mutations_select_to_slot(
   const uint32_t* counts_dev, const uint8_t* reference_index_dev, uint32_t n_positions, uint32_t n_symbols, double min_proportion,
   silo_gpu_row_slot* slot, void* stream
);
int silo_gpu_row_slot_wait(silo_gpu_row_slot* slot, const silo_gpu_mutation_row** out_rows, uint32_t* out_selected, void* stream);
/* Plain byte upload into a fresh device allocation (free with silo_gpu_free). */
int silo_gpu_upload_bytes(const void* src_host, size_t bytes, void** out_dev);

/* ---- K1: Mutations scan (mutations.cpp:64-164) ---------------------------------------------------
 * counts_out_dev[(p - pos_begin) * n_scan_symbols + s] += popcount(filter & {rows whose symbol at p is scan_symbols[s]})
 * for p in [pos_begin, pos_end), decoded from the bit-sliced scan planes (3 planes per nucleotide position, 5 per
 * amino-acid position; the scan symbols must be the 5 / 22 valid mutation symbols).  The buffer is ACCUMULATED into (the reference sums partitions into
 * one table, mutations.cpp:71,108); zero it with silo_gpu_memset_async before the first partition.
 * filter_dev == NULL means the full filter: like the reference, which then reads stored cardinalities
 * instead of intersecting (mutations.cpp:98-136), the totals of the unfiltered store are computed by one
 * scan on first use, kept on the device and added from then on (invalidated by append / generate).
 * A filter whose set bits fall into few 64-byte sectors (<= row_words / 16 by default, SILO_GPU_TUNE_SCAN_SPARSE_DIVISOR; and
 * fewer than the column tiles the dense scan cannot skip are worth: a clustered filter stays with the dense scan)
 * is served by a gather over just those sectors of the planes (K1s) — decided on the device, same counts, so that the
 * scan gets cheaper with the filter as roaring's and_cardinality does (mutations.cpp:139-164). */
int silo_gpu_mutations_scan(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint64_t* filter_dev,
   uint32_t pos_begin, uint32_t pos_end, uint32_t* counts_out_dev, void* stream
);
/* K1i, the compact scan index.  silo_gpu_store_finalize derives, per sequence store, two code planes per position (code
 * 1..3 = the three most frequent valid symbols AT THAT POSITION, 0 = anything else) plus the few rows whose valid symbol
 * is none of the three as explicit keys; the Mutations scan streams those 2 planes instead of the 3 / 5 full code planes
 * and adds the exceptions in one small pass — same counts.  Built only when the exceptions stay below 1/512 (nucleotides) or 1/170 (amino acids) of the cells
 * and the device memory is there (otherwise, and for every other consumer, the full planes serve).
 * silo_gpu_store_scan_planes: plane rows the scan reads per position (2 with the index, else 3 / 5);
 * silo_gpu_store_scan_escapes: number of exception keys (0 without the index). */
uint32_t silo_gpu_store_scan_planes(const silo_gpu_store* store, uint32_t seqstore_id);
uint64_t silo_gpu_store_scan_escapes(const silo_gpu_store* store, uint32_t seqstore_id);
/* The scan's escape pass reads the exception keys slice by slice of 2^17 sequences, packed to 4 bytes in granules of 4 096 keys:
 * a key's counter (position x scan symbols + symbol) relative to its granule's first.  A key more than 6 000 counters past it —
 * a stretch of positions with very few exceptions — is kept at 8 bytes in an overflow list that the scan counts in a launch of
 * its own.  silo_gpu_store_scan_overflow_keys: the keys of that list (0 for a store that is not finalized or has no
 * slice-major keys). */
uint64_t silo_gpu_store_scan_overflow_keys(const silo_gpu_store* store, uint32_t seqstore_id);
/* Plane rows (of Wp words each) the Mutations scan reads for positions [pos_begin, pos_end) of a sequence store: the
 * physical bytes of a scan are this x 8 Wp, plus the filter and 8 bytes per escape key. */
uint64_t silo_gpu_store_scan_rows(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t pos_begin, uint32_t pos_end);
/* Derived symbols.  At almost every position ONE valid symbol has nearly every row; the reference leaves that symbol's bitmap
 * out and rebuilds its count as |filter| - #missing - the other symbols' counts (position.cpp:102-127, mutations.cpp:74-95).
 * A finalized store whose missing symbol is kept as runs does the same: such a position stores no row and no key for its most
 * numerous symbol, and a scan derives that count from the filter's cardinality, the rows of the filter inside a run of the
 * missing symbol or with an ambiguity code, and the other symbols' counts — the same numbers.  silo_gpu_store_scan_planes is
 * then 0 (most positions have no row at all); a scan additionally reads the runs (12 bytes each) and the sparse keys (8 bytes
 * each): silo_gpu_store_scan_runs / _scan_sparse_keys (0 for a store without derived symbols). */
uint64_t silo_gpu_store_scan_runs(const silo_gpu_store* store, uint32_t seqstore_id);
uint64_t silo_gpu_store_scan_sparse_keys(const silo_gpu_store* store, uint32_t seqstore_id);
/* Finalizes ONE sequence store (silo_gpu_store_finalize does all that are left): its build-time planes are re-encoded into
 * the adaptive code planes and released.  A loader that fills the stores of a partition one after the other calls this
 * after each, so that their build-time planes are never resident together (10 M sequences: 112 GB for the nucleotide
 * genome alone).  No sequences can be appended to a finalized store. */
int silo_gpu_store_finalize_seqstore(silo_gpu_store* store, uint32_t seqstore_id);

/* K1 over several position ranges at once — the 12 genes of an AminoAcidMutations query, the segments of a segmented
 * genome, the sequence stores of several batched queries: every filter is applied to every range;
 * counts_out_dev[r * n_filters + q] is the table of filter q on range r, indexed from the range's first position and
 * ACCUMULATED into.  Ranges over stores of the same alphabet share launches (blocks are dealt to the ranges), and the
 * sparse-filter routing (K1s) looks at each filter once for all ranges.  Replaces the reference's loop over sequence
 * names in Mutations::execute (mutations.cpp:258-271). */
typedef struct silo_gpu_scan_range {
   uint32_t seqstore_id;
   uint32_t pos_begin;
   uint32_t pos_end;
} silo_gpu_scan_range;
int silo_gpu_mutations_scan_ranges(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   uint32_t* const* counts_out_dev, void* stream
);

/* The same scan for a caller that only wants the Mutations rows of a minimal proportion: min_proportion[q] (NULL = as
 * silo_gpu_mutations_scan_ranges) is the minProportion that filter q's table will be selected with.  For every range and filter
 * the row sums over the symbols, sum_s counts[p][s], are exact at every position, and so is every cell that
 * silo_gpu_mutations_select — with the store's reference symbols and that filter's proportion — emits from this table ALONE (a
 * table that other scans are accumulated into as well, the partitions of a database, needs the exact entry).  Other cells may
 * not be: at a position whose most numerous symbol is derived (SILO_GPU_TUNE_COMPACT_INDEX) and is the reference symbol, the
 * scan leaves out (position, symbol) groups too small in the whole store to reach the proportion under the filter — their
 * escape keys, whole granules of the key stream at a time, and their one-hot plane rows, a row at a time, where the derived symbol holds the majority of the position's valid rows — and their rows are
 * counted on the derived symbol instead, which is never reported.  A proportion of 0 (or outside (0, 1]), a store without gap
 * events, SILO_GPU_TUNE_GAP_EVENTS < 0 or SILO_GPU_TUNE_PRUNE_KEYS < 0: exactly silo_gpu_mutations_scan_ranges. */
int silo_gpu_mutations_scan_ranges_min_proportion(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   const double* min_proportion /* [n_filters] or NULL */, uint32_t* const* counts_out_dev, void* stream
);
/* That scan and the row selection (K4) in one call, for a caller whose scan is the ONLY writer of each filter's count table and
 * whose only reader is the selection: a Mutations query over one partition.  Per filter a sink: its table (total_positions x
 * n_symbols words; every counts_out_dev[r * n_filters + q] points into table q), the reference symbols of the table's
 * positions (as silo_gpu_mutations_select), and the row slot its rows go to.  min_proportion[q] serves the scan's pruning and
 * the selection alike (NULL = 0 for every filter).
 * The tables are OVERWRITTEN, not accumulated into: on return (in stream order) table q holds exactly this call's counts — as
 * silo_gpu_mutations_scan_ranges_min_proportion into a cleared table —, whatever it held before; the caller does not clear it.
 * The rows of filter q arrive in its slot as from silo_gpu_mutations_select_to_slot (silo_gpu_row_slot_wait; the number of
 * selected cells may exceed the capacity, the table is then complete for the caller's fallback).
 * Where every range goes through the finish kernel of a scan with derived symbols (k_finish_scan: one alphabet, rows of at least
 * 1 024 words, a store with derived symbols and gap events) and the ranges of the call tile [0, total_positions) of every
 * table exactly and alike, that kernel stores the cells and selects the rows from the registers it holds them in: no fill
 * launch, no selection launch.  Otherwise — and with SILO_GPU_TUNE_FUSED_SELECT < 0 — the call clears the tables, scans and
 * launches the selection, as a caller of the other entries would. */
typedef struct silo_gpu_select_sink {
   uint32_t* table_dev;
   uint32_t total_positions;
   uint32_t n_symbols;
   const uint8_t* reference_index_dev; /* [total_positions] */
   silo_gpu_row_slot* slot;
} silo_gpu_select_sink;
int silo_gpu_mutations_scan_select(
   const silo_gpu_store* store, const silo_gpu_scan_range* ranges, uint32_t n_ranges, const uint64_t* const* filters_dev, uint32_t n_filters,
   const double* min_proportion /* [n_filters] or NULL */, uint32_t* const* counts_out_dev, const silo_gpu_select_sink* sinks /* [n_filters] */, void* stream
);
/* How many granules (4 096 keys) of the store's slice-major escape keys the scan above skips for ONE filter of `cardinality`
 * rows at `min_proportion`, and how many there are: the kernel's rule applied to the host copies of the store's bounds. */
int silo_gpu_store_scan_prunable_granules(
   const silo_gpu_store* store, uint32_t seqstore_id, uint32_t cardinality, double min_proportion, uint64_t* out_skippable, uint64_t* out_total
);
/* Its twin for the one-hot plane rows: how many of them that scan skips for ONE filter of `cardinality` rows at `min_proportion`,
 * and how many the store has (a store without bounds per row: 0 of them). */
int silo_gpu_store_scan_prunable_rows(
   const silo_gpu_store* store, uint32_t seqstore_id, uint32_t cardinality, double min_proportion, uint64_t* out_skippable, uint64_t* out_total
);
/* The end runs of the gap symbol '-' (a sequence that has not begun yet, or has already ended), which a Mutations scan counts
 * instead of reading the one-hot rows of '-' at the alignment's ragged ends (SILO_GPU_TUNE_END_RUNS): the one-hot rows the scan
 * leaves out (covered rows), the end events it streams instead (one where a sequence's leading run ends, one where its trailing
 * run begins) and the residual keys (set bits of the covered rows outside every end run: interior deletions).  All 0 for a store
 * without them: built in two passes, imported, of more than 67 M rows, without derived symbols, or where no row is covered.
 * The store itself keeps the rows: every other reader finds them where they are. */
uint64_t silo_gpu_store_scan_covered_rows(const silo_gpu_store* store, uint32_t seqstore_id);
uint64_t silo_gpu_store_scan_end_events(const silo_gpu_store* store, uint32_t seqstore_id);
uint64_t silo_gpu_store_scan_residual_keys(const silo_gpu_store* store, uint32_t seqstore_id);

/* ---- K7: grouped mutation counts (MutationsOverTime) -------------------------------------------------
 * For each of n_mutations listed cells (positions[m] 0-based in the store, symbols[m] a VALID mutation symbol id of the
 * store's alphabet) and each of n_ranges date ranges (range_bounds[2r], range_bounds[2r + 1] = from, to, encoded dates
 * as in K5, BOTH ends inclusive, 0 / 0xFFFFFFFF where unbounded; pairwise disjoint; rows whose date is NULL (0) fall in no
 * range), over the rows selected by filter_dev (NULL = all rows) whose date_column_dev value lies in the range:
 *     out_dev[(m * n_ranges + r) * 2 + 0] += rows whose symbol at positions[m] is symbols[m]            (count)
 *     out_dev[(m * n_ranges + r) * 2 + 1] += rows with any valid mutation symbol at positions[m]        (coverage)
 * exactly K1's cell counts[p][s] and its sum over the valid symbols under the filter And(filter, date in range), for every
 * store layout (identity / code planes with escape keys, one-hot rows with a derived symbol, runs of the missing symbol,
 * sparse or extra ambiguity planes).  ACCUMULATED into, like K1: partitions add up in one table.
 * group_scratch_dev: device memory of SILO_GPU_GROUPED_SCRATCH_BYTES(row_words, n_ranges, n_mutations) bytes, 16-byte
 * aligned; its first row_words * 64 uint16 hold each row's range (0xFFFF = none) after the call.  Uploads its small host
 * tables and waits for them (one stream synchronisation), then launches K7 on `stream` without waiting.
 * Fails with SILO_GPU_ERR_INVALID_ARGUMENT for more than SILO_GPU_MAX_DATE_RANGES ranges or SILO_GPU_MAX_GROUPED_MUTATIONS
 * cells, a position out of bounds, a symbol that is not a valid mutation symbol, from > to, or overlapping ranges. */
#define SILO_GPU_MAX_DATE_RANGES 1024
#define SILO_GPU_MAX_GROUPED_MUTATIONS 4096
#define SILO_GPU_GROUPED_SCRATCH_BYTES(row_words, n_ranges, n_mutations)                                                    \
   ((size_t)(row_words) * 128u + (size_t)(n_mutations) * 32u + (size_t)(n_ranges) * 16u +                                   \
    (size_t)(n_ranges) * 4u * (1u + 3u * (size_t)(n_mutations)) + 1024u)
int silo_gpu_mutations_grouped(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint64_t* filter_dev, const uint32_t* date_column_dev, const uint32_t* range_bounds,
   uint32_t n_ranges, const uint32_t* positions, const uint32_t* symbols, uint32_t n_mutations, void* group_scratch_dev, uint32_t* out_dev,
   void* stream
);

/* ---- K8: grouped filter counts (QueriesOverTime) ----------------------------------------------------
 * For each of n_filters row bitsets (filters_dev: a HOST array of device pointers, row_words words each; a NULL entry = all
 * rows) and each of n_ranges date ranges (range_bounds, date_column_dev and the rules for ranges exactly as for K7: both ends
 * inclusive, pairwise disjoint, NULL dates in no range), over the rows selected by base_filter_dev (NULL = all rows):
 *     out_dev[f * n_ranges + r] += |{row < sequence_count : base(row) and filter_f(row) and from_r <= date(row) <= to_r}|
 * ACCUMULATED into, like K1 and K7.  Bits of a filter or of the base at or past sequence_count never count.
 * scratch_dev: device memory of SILO_GPU_FILTERS_GROUPED_SCRATCH_BYTES(row_words, n_ranges, n_filters) bytes, 16-byte aligned;
 * its first row_words * 64 uint16 hold each row's range under the base filter (0xFFFF = none) after the call.  Uploads its
 * small host tables and waits for them (one stream synchronisation), then makes two launches on `stream` without waiting.
 * No ranges or no filters: success, nothing launched.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT for more than
 * SILO_GPU_MAX_DATE_RANGES ranges or SILO_GPU_MAX_GROUPED_FILTERS filters, from > to, overlapping ranges, a NULL date column,
 * scratch, table or filter array, or a store without rows. */
#define SILO_GPU_MAX_GROUPED_FILTERS 2048
#define SILO_GPU_FILTERS_GROUPED_SCRATCH_BYTES(row_words, n_ranges, n_filters)                                              \
   ((size_t)(row_words) * 128u + (size_t)(n_filters) * 8u + (size_t)(n_ranges) * 16u + 1024u)
int silo_gpu_filters_grouped(
   const silo_gpu_store* store, const uint64_t* base_filter_dev, const uint32_t* date_column_dev, const uint32_t* range_bounds, uint32_t n_ranges,
   const uint64_t* const* filters_dev, uint32_t n_filters, void* scratch_dev, uint32_t* out_dev, void* stream
);

/* ---- K9: pair counts of two filter lists (CrossTabulation) ------------------------------------------
 * out_dev is a table [out_rows][out_cols] of uint32, ACCUMULATED into, like K1, K7 and K8.  For every i < n_rows and j < n_cols,
 * with ri(i) = row_index[i] and cj(j) = col_index[j]:
 *     out_dev[ri(i) * out_cols + cj(j)] += |{row < sequence_count : base(row) and rowfilter_i(row) and colfilter_j(row)}|
 * row_filters_dev, col_filters_dev: HOST arrays of device pointers, row_words words each; a NULL entry = all rows.
 * base_filter_dev: NULL = all rows.  row_index, col_index: HOST arrays that say where filter i / j lands in the table (NULL =
 * identity); entries must be < out_rows / < out_cols and distinct within their array.  A caller leaves out a filter that selects
 * no row (its cells stay untouched) or fills a large table in sub-blocks with them.  The same pointer may stand on both sides:
 * cell (i, i) is then that filter's cardinality under the base.  Bits of the base, a row filter or a column filter at or past
 * sequence_count never count: NULL x NULL under a NULL base is exactly sequence_count.
 * scratch_dev: device memory of SILO_GPU_FILTERS_CROSS_SCRATCH_BYTES(n_rows, n_cols) bytes, 16-byte aligned.  Uploads its
 * pointer and index tables there and waits for them (one stream synchronisation), then makes one launch on `stream` without
 * waiting: a block counts SILO_GPU_CROSS_TILE x SILO_GPU_CROSS_TILE pairs over SILO_GPU_CROSS_CHUNK_WORDS row words, so every
 * bitset is read once per SILO_GPU_CROSS_TILE filters of the other side.
 * n_rows == 0 or n_cols == 0: success, nothing launched.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT for more than
 * SILO_GPU_MAX_CROSS_FILTERS filters on a side, a NULL table, scratch or filter array, an index out of bounds or given twice, or
 * a store without rows. */
#define SILO_GPU_MAX_CROSS_FILTERS 1024 /* per side */
#define SILO_GPU_CROSS_TILE 8
#define SILO_GPU_CROSS_CHUNK_WORDS 1024
#define SILO_GPU_FILTERS_CROSS_SCRATCH_BYTES(n_rows, n_cols) (((size_t)(n_rows) + (size_t)(n_cols)) * 16u + 1024u)
int silo_gpu_filters_cross(
   const silo_gpu_store* store, const uint64_t* base_filter_dev, const uint64_t* const* row_filters_dev, const uint32_t* row_index, uint32_t n_rows,
   const uint64_t* const* col_filters_dev, const uint32_t* col_index, uint32_t n_cols, void* scratch_dev, uint32_t* out_dev, uint32_t out_rows,
   uint32_t out_cols, void* stream
);

/* ---- K10: pairwise distances of rows of characters (DistanceMatrix) ----------------------------------
 * Neither entry takes a store (like silo_gpu_mutations_select): they start from the characters that
 * silo_gpu_reconstruct_sequences writes for every store layout, chars_dev[r * positions + p].
 * silo_gpu_distance_pack turns every row into SILO_GPU_DISTANCE_PLANES(alphabet) bit planes over POSITIONS of
 * SILO_GPU_DISTANCE_WORDS(positions) words each, planes_dev[(r * PLANES + k) * WORDS + w], bit b of word w = position 64 w + b:
 *     plane 0      the character is a valid mutation symbol of the alphabet (nucleotide "-ACGT", amino acid
 *                  "-ACDEFGHIKLMNPQRSTVWY*": what Mutations counts);
 *     plane 1 + k  bit k of that symbol's index in the string above, 0 where the position is not valid.
 * Every other byte — N, X, the ambiguity codes, bytes that are no symbol at all — is not valid.  Every word of every row's slot
 * is written, the bits at or past `positions` as zeros: the caller never clears the buffer.
 * silo_gpu_distance_pairs WRITES (no accumulation, no atomics) for every pair i <= j < n_rows
 *     out_dev[(i * n_rows + j) * 2]     = differing = sum_w popcount(valid_i & valid_j & OR_k (code_i,k ^ code_j,k))
 *     out_dev[(i * n_rows + j) * 2 + 1] = compared  = sum_w popcount(valid_i & valid_j)
 * so the diagonal holds (0, valid positions of row i); cells with i > j are never touched.  Only tiles of SILO_GPU_DISTANCE_TILE x
 * SILO_GPU_DISTANCE_TILE pairs on or above the diagonal are launched; a block stages SILO_GPU_DISTANCE_CHUNK_WORDS words of every
 * plane of its 2 x SILO_GPU_DISTANCE_TILE rows in LDS at a time, so a packed word is read from memory once per tile of the other
 * side.  Each pair belongs to one thread of one block: the result does not depend on how the blocks are scheduled.
 * Both make their launch on `stream` and return without waiting.  n_rows == 0 or positions == 0: success, nothing launched.
 * Fail with SILO_GPU_ERR_INVALID_ARGUMENT for an alphabet other than the two, a NULL buffer or more than
 * SILO_GPU_MAX_DISTANCE_ROWS rows. */
#define SILO_GPU_MAX_DISTANCE_ROWS 2048
#define SILO_GPU_DISTANCE_PLANES(alphabet) ((alphabet) == SILO_GPU_ALPHABET_AMINO_ACID ? 6u : 4u) /* 1 valid plane + 5 / 3 code bits */
#define SILO_GPU_DISTANCE_WORDS(positions) (((positions) + 63u) / 64u)
#define SILO_GPU_DISTANCE_TILE 16
#define SILO_GPU_DISTANCE_CHUNK_WORDS 32
int silo_gpu_distance_pack(int alphabet, const char* chars_dev, uint32_t n_rows, uint32_t positions, uint64_t* planes_dev, void* stream);
int silo_gpu_distance_pairs(int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, uint32_t* out_dev, void* stream);

/* ---- K12: which pairs are within a bound, and the connected components of that relation (Clusters) ---
 * Neither entry takes a store.  silo_gpu_distance_within reads planes as silo_gpu_distance_pack leaves them (that entry keeps its
 * own limit of SILO_GPU_MAX_DISTANCE_ROWS rows per call: the caller packs in batches into one plane buffer) and WRITES a bit matrix
 * of AW = SILO_GPU_ADJACENCY_WORDS(n_rows) words per row, adjacency_dev[i * AW + (j >> 6)] bit (j & 63):
 *     bit (i, j) = i != j && i < n_rows && j < n_rows && differing(i, j) <= max_distance && compared(i, j) >= min_compared
 * with differing / compared as silo_gpu_distance_pairs counts them.  max_distance == UINT32_MAX: no bound on the distance;
 * min_compared == 0: none on the compared positions.  The matrix is symmetric, its diagonal is clear and the bits at or past n_rows
 * are zero.  Every one of the n_rows * AW words is written once and nothing behind them is touched: the caller never clears the
 * buffer.  No atomics: the words do not depend on how the blocks are scheduled.
 * Two launches on `stream`, no waiting.  k_distance_within: a block of 256 threads owns a tile of SILO_GPU_WITHIN_TILE_ROWS rows x
 * SILO_GPU_WITHIN_TILE_COLS columns (= one word of 4 rows per wave, four pairs per thread in registers) and stages
 * SILO_GPU_WITHIN_CHUNK_WORDS words of every plane of its 16 + 64 rows in LDS at a time; only the tiles whose word is at or right
 * of the word that holds the diagonal are launched, and a wave's ballot is the finished word.  After every chunk the block stops if
 * none of its pairs can still be linked (differing only grows along the row; a pair with a row at or past n_rows and a pair i == j
 * count as out from the start): its words are then zeros.  The words are exact either way; only the time depends on the data.
 * k_adjacency_mirror fills the words left of the diagonal's word from the transposed 64 x 64 blocks right of it.
 * n_rows == 0: success, nothing launched.  positions == 0: every pair has compared = differing = 0, and the matrix of that is
 * written.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an alphabet other than the two, a NULL buffer or more
 * than SILO_GPU_MAX_CLUSTER_ROWS rows.
 * silo_gpu_adjacency_components takes such a matrix, which must be symmetric (bits at or past n_rows in a row's last word are
 * ignored: they never index the labels), and WRITES labels_dev[i] = the lowest j in the connected component of i, for i < n_rows,
 * and, unless rounds_dev is NULL, *rounds_dev = the rounds it ran (at most n_rows).  One launch of ONE block of
 * SILO_GPU_COMPONENTS_THREADS threads on `stream`, no waiting: the labels live in LDS (4 bytes per row); a round gives every row
 * to a wave, which takes the lowest label among the row's neighbours and lowers (atomicMin in LDS) the row's label and the label
 * of the row's old label to it, then every label jumps to its label's label until none changes; a round that lowers nothing ends
 * the loop, which n_rows bounds whatever the input.  Labels only fall and every label is a row of its row's own component, so the
 * labels at the end do not depend on the order of the atomics (the round count may).  The matrix is read once per round.
 * n_rows == 0: success, nothing launched or written.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL
 * matrix, NULL labels or more than SILO_GPU_MAX_CLUSTER_ROWS rows. */
#define SILO_GPU_MAX_CLUSTER_ROWS 8192
#define SILO_GPU_ADJACENCY_WORDS(n_rows) (((n_rows) + 63u) / 64u)
#define SILO_GPU_WITHIN_TILE_ROWS 16
#define SILO_GPU_WITHIN_TILE_COLS 64
#define SILO_GPU_WITHIN_CHUNK_WORDS 16
#define SILO_GPU_COMPONENTS_THREADS 1024
int silo_gpu_distance_within(
   int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, uint32_t max_distance, uint32_t min_compared,
   uint64_t* adjacency_dev, void* stream
);
int silo_gpu_adjacency_components(const uint64_t* adjacency_dev, uint32_t n_rows, uint32_t* labels_dev, uint32_t* rounds_dev, void* stream);

/* ---- K13: the distances of the pairs within a bound, and the minimum spanning forest of that graph (MinimumSpanningTree) ---
 * No entry takes a store.  An EDGE is a pair i != j of rows < n_rows with differing(i, j) <= max_distance and compared(i, j) >=
 * min_compared, both as silo_gpu_distance_pairs counts them (max_distance == UINT32_MAX: no bound; min_compared == 0: none): the
 * pairs whose bit silo_gpu_distance_within sets.
 * silo_gpu_distance_weights reads planes as silo_gpu_distance_pack leaves them and WRITES the full symmetric matrix
 *     weights_dev[i * n_rows + j] = differing(i, j) where (i, j) is an edge, UINT32_MAX where it is not and on the diagonal.
 * Every one of the n_rows * n_rows cells is written once and nothing behind them is touched: the caller never clears the buffer.
 * No atomics: the cells do not depend on how the blocks are scheduled.  One launch on `stream`, no waiting: the tiles, the LDS
 * staging and the early exit are those of k_distance_within (the two kernels share the walk); a block whose pairs have all passed
 * the bound stops, and its cells are UINT32_MAX.  Only the tiles at or right of the diagonal's 64 x 64 block are launched; a tile
 * right of it writes its transpose as well.  n_rows == 0: success, nothing launched.  positions == 0: every pair has compared =
 * differing = 0, and the matrix of that is written.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an alphabet
 * other than the two, a NULL buffer or more than SILO_GPU_MAX_SPANNING_ROWS rows.
 * silo_gpu_spanning_forest takes such a matrix (UINT32_MAX: no edge; the diagonal is ignored) and WRITES *count_dev = the number
 * of edges of its minimum spanning forest and edges_dev[0 .. count) = their keys
 *     SILO_GPU_SPANNING_KEY(weight, i, j) = weight << 26 | i << 13 | j,   i < j,
 * ASCENDING.  Edges are ordered by that key, a strict order, so the forest is unique and the output a pure function of the
 * matrix; cutting it at any d leaves the single-linkage clusters at d.  Entries at or past the count are untouched (room for
 * n_rows - 1 keys is enough).  One launch of ONE block of SILO_GPU_SPANNING_THREADS threads on `stream`, no waiting: Prim's
 * algorithm with a restart — a thread keeps the best key of each of its <= 8 vertices in registers, a step reads one row of the
 * matrix, takes the block-wide minimum and moves one vertex into the forest (with no key left, the lowest vertex outside it,
 * without an edge) — then a bitonic sort of the keys in LDS.  Exactly n_rows - 1 steps whatever the matrix holds, and nothing read
 * from the matrix is used as an index; for an asymmetric matrix the output is unspecified (but count <= n_rows - 1 and i < j <
 * n_rows hold).  n_rows == 0: success, nothing launched or written.  n_rows == 1: count 0.  Fails with
 * SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer or more than SILO_GPU_MAX_SPANNING_ROWS rows.
 * silo_gpu_distance_listed_pairs WRITES for every e < min(*count_dev, max_pairs), with (i, j) the low 26 bits of edges_dev[e],
 *     out_dev[2 e] = differing(i, j),   out_dev[2 e + 1] = compared(i, j)
 * — a wave per pair — and (UINT32_MAX, UINT32_MAX), without reading a plane, where i or j is >= n_rows.  Entries at or past the
 * count are untouched.  One launch on `stream`, no waiting (none for max_pairs == 0).  Fails with SILO_GPU_ERR_INVALID_ARGUMENT,
 * nothing written, for an alphabet other than the two, a NULL buffer or more than SILO_GPU_MAX_SPANNING_ROWS rows. */
#define SILO_GPU_MAX_SPANNING_ROWS 8192
#define SILO_GPU_SPANNING_THREADS 1024
#define SILO_GPU_SPANNING_KEY_ROW_BITS 13    /* a row of the key: SILO_GPU_MAX_SPANNING_ROWS == 1 << 13 */
#define SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT 26 /* two rows below the weight */
#define SILO_GPU_SPANNING_KEY(weight, i, j) \
   (((uint64_t)(weight) << SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT) | ((uint64_t)(i) << SILO_GPU_SPANNING_KEY_ROW_BITS) | (uint64_t)(j))
int silo_gpu_distance_weights(
   int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, uint32_t max_distance, uint32_t min_compared,
   uint32_t* weights_dev, void* stream
);
int silo_gpu_spanning_forest(const uint32_t* weights_dev, uint32_t n_rows, uint64_t* edges_dev, uint32_t* count_dev, void* stream);
int silo_gpu_distance_listed_pairs(
   int alphabet, const uint64_t* planes_dev, uint32_t n_rows, uint32_t positions, const uint64_t* edges_dev, const uint32_t* count_dev,
   uint32_t max_pairs, uint32_t* out_dev, void* stream
);

/* ---- K14: the distances of one set of rows against another, and the k lowest of every row (NearestAmong) ---
 * Neither entry takes a store.  A column j is ELIGIBLE for a row i when j != self_column_dev[i], differing(i, j) <= max_distance
 * and compared(i, j) >= min_compared, both as silo_gpu_distance_pairs counts them for row i of the row planes and row j of the
 * column planes (max_distance == UINT32_MAX: no bound; min_compared == 0: none).
 * silo_gpu_distance_cross reads two plane buffers as silo_gpu_distance_pack leaves them — n_rows <= SILO_GPU_MAX_CROSS_ROWS rows of
 * the one, n_columns <= SILO_GPU_MAX_CROSS_COLUMNS rows of the other, the same alphabet and positions; the same buffer may stand on
 * both sides — and WRITES the rectangle
 *     cells_dev[(i * n_columns + j) * 2 + 0 .. 1] = (differing, compared)       where j is eligible for i,
 *                                                   (UINT32_MAX, UINT32_MAX)   where it is not.
 * self_column_dev: n_rows values in device memory, the column that is the same row as row i and is never eligible for it; NULL:
 * none; a value at or past n_columns names no column.  Every one of the n_rows * n_columns cells is written once and nothing behind
 * them is touched: the caller never clears the buffer.  No atomics: the cells do not depend on how the blocks are scheduled.  One
 * launch on `stream`, no waiting: the plain grid of n_rows / 16 x n_columns / 64 tiles (rounded up; no symmetry, no transpose), the
 * tile, the LDS staging and the early exit of k_distance_within (the kernels share the walk); a block whose pairs have all passed
 * max_distance stops, and its cells are the UINT32_MAX pairs.  A thread stores its four cells as 8-byte stores: cells_dev is 8-byte
 * aligned.  n_rows == 0 or n_columns == 0: success, nothing launched.  positions == 0: every pair has compared = differing = 0, and
 * the cells of that are written.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an alphabet other than the two, a
 * NULL plane or cell buffer, or either count above its limit.
 * silo_gpu_nearest_columns takes such cells (a cell whose first word is UINT32_MAX is not eligible) and WRITES per row i < n_rows
 *     counts_dev[i] = min(k, eligible cells of row i)
 *     out_dev[(i * k + r) * 3 + 0 .. 2] = column, distance, compared     for r < counts_dev[i], ascending by (distance, column)
 * — a strict order, so the lists are unique and two calls give the same output.  Entries of a row's list at or past its count are
 * untouched.  One launch on `stream`, no waiting: a block of SILO_GPU_NEIGHBOUR_THREADS threads per row keeps the keys
 *     distance << SILO_GPU_NEIGHBOUR_KEY_COLUMN_BITS | column
 * of its <= 8 cells per thread in registers (UINT64_MAX: not eligible) and runs exactly min(k, n_columns) rounds of a block-wide
 * minimum (the forest kernel's reduction); a round lists one column, whose owner retires its key, or nothing at all.  Nothing read
 * from the cells is used as an index; no atomics, no spin.  n_rows == 0: success, nothing launched.  n_columns == 0: the counts are
 * written as 0.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, k == 0, k >
 * SILO_GPU_MAX_NEIGHBOUR_COLUMNS or either count above its limit. */
#define SILO_GPU_MAX_CROSS_ROWS 2048      /* the rows of the rectangle: == SILO_GPU_MAX_DISTANCE_ROWS */
#define SILO_GPU_MAX_CROSS_COLUMNS 8192   /* its columns: == SILO_GPU_MAX_CLUSTER_ROWS */
#define SILO_GPU_MAX_NEIGHBOUR_COLUMNS 64 /* k of silo_gpu_nearest_columns */
#define SILO_GPU_NEIGHBOUR_THREADS 1024
#define SILO_GPU_NEIGHBOUR_KEY_COLUMN_BITS 13 /* the column of a key: SILO_GPU_MAX_CROSS_COLUMNS == 1 << 13 */
int silo_gpu_distance_cross(
   int alphabet, const uint64_t* row_planes_dev, uint32_t n_rows, const uint64_t* column_planes_dev, uint32_t n_columns, uint32_t positions,
   const uint32_t* self_column_dev, uint32_t max_distance, uint32_t min_compared, uint32_t* cells_dev, void* stream
);
int silo_gpu_nearest_columns(
   const uint32_t* cells_dev, uint32_t n_rows, uint32_t n_columns, uint32_t k, uint32_t* out_dev, uint32_t* counts_dev, void* stream
);

/* ---- K15: the consensus call of count tables (Consensus / AminoAcidConsensus) --------------------------
 * Takes no store.  counts_dev holds n_tables <= SILO_GPU_MAX_CONSENSUS_TABLES tables back to back, n_positions x n_symbols words
 * each (n_symbols = 5 "-ACGT" / 22 "-ACDEFGHIKLMNPQRSTVWY*"): what silo_gpu_mutations_scan accumulates.  reference_index_dev is as
 * for silo_gpu_mutations_select, n_positions bytes shared by every table (0xFF: the reference symbol is not a valid one).
 * Per table and position, with c[s] the counts and depth = sum_s c[s] (no wrap is defined: depth <= UINT32_MAX):
 *     depth < min_depth                         the missing symbol 'N' / 'X'; the position is LOW COVERAGE
 *     otherwise need = (uint32_t)ceil((double)depth * threshold)   (IEEE double, as K4 computes its bound), and the call's symbols
 *     are those with c[s] >= cut, where cut is the highest count whose symbols, with every symbol above it, sum to >= need:
 *     the shortest prefix by descending count that reaches need, extended by every symbol tied with its last — never a matter of
 *     symbol order.  cut > 0: a symbol nobody has is never in the call.
 *       one symbol       its character ('-' included: the position is DELETED)
 *       several symbols  the position is AMBIGUOUS: nucleotides all of ACGT — the IUPAC code of the set (M AC, R AG, W AT, S CG,
 *                        Y CT, K GT, V ACG, H ACT, D AGT, B CGT, N ACGT); nucleotides with '-' among them — 'N'; amino acids — 'X'
 * WRITES out_chars_dev[t * n_positions + p], every character once, and out_summary_dev[t * 4 + 0 .. 3] = the table's ambiguous,
 * low-coverage and deleted positions and its DIFFERENCES: positions neither low coverage nor ambiguous whose symbol's index is
 * not reference_index_dev[p].  Nothing is accumulated into: the call clears the summary words itself, on `stream`, and the
 * blocks add integers to them, so two calls give the same bytes; the caller clears nothing.  One kernel launch serves all tables
 * (a block of SILO_GPU_CONSENSUS_THREADS threads per as many positions of one table, staged through LDS; a thread per position; no
 * scratch memory), returns without waiting.  counts_dev is 4-byte aligned (16-byte loads are used where they stay inside the tables).
 * n_tables == 0 or n_positions == 0: success, nothing written.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an
 * alphabet other than the two, a NULL pointer, a threshold outside (0, 1] or NaN, min_depth == 0 or n_tables above the limit. */
#define SILO_GPU_MAX_CONSENSUS_TABLES 64
#define SILO_GPU_CONSENSUS_THREADS 256
int silo_gpu_consensus_call(
   int alphabet, const uint32_t* counts_dev, uint32_t n_tables, uint32_t n_positions, const uint8_t* reference_index_dev, double threshold,
   uint32_t min_depth, char* out_chars_dev, uint32_t* out_summary_dev, void* stream
);

/* ---- K16: the symbols of every row at listed positions, and their tuple ids (Haplotypes / AminoAcidHaplotypes) ---
 * silo_gpu_position_symbols reads the symbol of EVERY row at n_positions <= SILO_GPU_MAX_HAPLOTYPE_POSITIONS positions (`positions`
 * in HOST memory, 0-based; the same position may be listed twice) off the store's own layout and WRITES every byte of
 *     out_symbols_dev[c * row_words * 64 + r] = the symbol id of row r at positions[c]
 * in the store's own enumeration — the one silo_gpu_store_plane takes: valid symbols, the missing symbol, ambiguity codes.  Rows at
 * or past sequence_count get SILO_GPU_SYMBOL_NONE.  So does a real row that nothing stored claims at a position without a derived
 * symbol (an imported store may hold such rows); those cells are counted into *out_unresolved_dev, which the entry clears itself
 * with a memset on `stream` ahead of its launches: the caller clears nothing, and a second call gives the same bytes.  Work follows
 * what the store holds, one pass per kind of stored thing (the decomposition of K7 and K11): the plane pass (grid = rows / 256 x
 * n_positions, a thread per row, a wave per row word: wave-uniform 8-byte plane loads, 64 consecutive bytes stored; codes and
 * one-hot rows, the derived symbol of a derived position, extra planes), then on the same stream the override passes with plain
 * byte stores — the escape keys of the listed positions' ranges of the position-major list, the runs of the missing symbol (a
 * thread per run, a binary search of the sorted listed positions held in the kernel arguments), the sparse keys of the listed
 * positions' ranges — and the count of the bytes still SILO_GPU_SYMBOL_NONE among real rows (a ballot per wave, one integer add per
 * block that found any).  A cell holds one symbol and finalize stores it in one place, so no two threads write the same byte.
 * No index is taken from a key or a run without a check against the listed positions and sequence_count; no spin, no float.  No
 * table is uploaded (everything per position fits the kernel arguments): all launches go on `stream`, the entry returns without
 * waiting and never synchronises.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, a store that is
 * not finalized, a seqstore_id or a position out of range, n_positions == 0 or above the maximum.
 * silo_gpu_haplotype_ids takes such columns (no store, like K10 and silo_gpu_nearest_rows) and WRITES ceil(n_positions /
 * SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN) id columns of row_words * 64 words (out_ids_dev: their device addresses, an array in
 * HOST memory):
 *     out_ids_dev[j][r] = sum_{i < m} symbols[6 j + i][r] * n_symbols^(m - 1 - i),     m = min(6, n_positions - 6 j)
 * the first listed position the most significant digit — columns for silo_gpu_group_count / silo_gpu_group_count_hashed with the
 * cardinalities n_symbols^m.  A row with a byte at or past n_symbols (SILO_GPU_SYMBOL_NONE, or whatever no symbol id can be) and
 * every row at or past sequence_count gets 0 in ALL columns: an id never leaves its column's tuple space.  Where out_rows_dev is
 * not NULL every one of its row_words words is written:
 *     bit r = r < sequence_count && filter bit r (filter_dev NULL: every row) && every listed symbol of r is in complete_symbols
 * (bit s of the mask: symbol s counts as complete; a byte of 32 or more is in the mask only where the mask is all ones), so the
 * bits at or past sequence_count are 0 whatever the filter holds there, and with complete_symbols all ones the word is the filter
 * masked to real rows.  One launch on `stream` (a thread per row, a wave's ballot is the word; no atomics), returns without
 * waiting.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL symbol buffer, column array or column,
 * n_symbols == 0 or above 32, n_positions == 0 or above the maximum, row_words == 0 or sequence_count > row_words * 64. */
#define SILO_GPU_MAX_HAPLOTYPE_POSITIONS 12
#define SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN 6 /* 16^6 = 2^24, 25^6 < 2^28: an id column is a uint32 */
int silo_gpu_position_symbols(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint32_t* positions /* host, 0-based */, uint32_t n_positions,
   uint8_t* out_symbols_dev /* [n_positions][row_words * 64] */, uint32_t* out_unresolved_dev /* 1 word */, void* stream
);
int silo_gpu_haplotype_ids(
   const uint8_t* symbols_dev, uint32_t n_positions, uint32_t row_words, uint32_t sequence_count, uint32_t n_symbols,
   uint32_t complete_symbols /* bit s: symbol s counts as complete */, const uint64_t* filter_dev /* NULL = all rows */,
   uint32_t* const* out_ids_dev /* ceil(n_positions / 6) columns of row_words * 64 */, uint64_t* out_rows_dev /* row_words words, or NULL */,
   void* stream
);

/* ---- K17: the comparison of count tables (MutationsComparison / AminoAcidMutationsComparison) -----------
 * Takes no store.  counts_dev and reference_index_dev are as for silo_gpu_consensus_call: 2 <= n_tables <=
 * SILO_GPU_MAX_COMPARISON_TABLES tables back to back, n_positions x n_symbols words each (n_symbols = 5 / 22), 4-byte aligned; the
 * reference's symbol index per position, 0xFF for none.  With c[t][p][s] a cell and cov[t][p] = sum_s c[t][p][s] (no wrap is
 * defined):
 *     table t PASSES (p, s)   iff cov[t][p] > 0 and c[t][p][s] > bound, bound = 0 if min_proportion == 0, else
 *                             (uint32_t)(ceil((double)cov[t][p] * min_proportion) - 1): the arithmetic of silo_gpu_mutations_select
 *     difference(p, s)        = the highest minus the lowest of (double)c[t][p][s] / (double)cov[t][p] (IEEE division) over the
 *                             tables with cov[t][p] > 0; 0.0 where fewer than two tables are covered
 *     (p, s) is SELECTED      iff s != reference_index_dev[p], some table passes it and difference(p, s) >= min_difference
 * WRITES out_dev, 4 + capacity * 2 + capacity * n_tables * 2 words:
 *     4 header words          word 0 = the number of selected cells, which may exceed `capacity`; words 1 .. 3 = 0
 *     capacity records        {uint32 position, uint32 symbol}: the selected cells that found a slot, in no particular order
 *     capacity * n_tables cells   for record slot i and table t, {count, coverage} = {c[t][p][s], cov[t][p]} at word
 *                             4 + capacity * 2 + (i * n_tables + t) * 2
 * Past `capacity` only the counter advances, as in silo_gpu_mutations_select; slots at or past min(word 0, capacity) are not
 * written.  capacity == 0 is legal: the count alone.  The entry clears the header itself, on `stream`, and the threads add
 * integers to word 0, so two calls give the same bytes once the records are put in order; the caller clears nothing.  One kernel
 * launch (a block of SILO_GPU_COMPARE_THREADS threads per as many positions, a thread per position, every table's slab of the
 * block staged through LDS; no scratch memory), returns without waiting.  n_positions == 0: success, only the header cleared.
 * Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an alphabet other than the two, a NULL pointer, n_tables below 2 or
 * above the limit, or min_proportion or min_difference outside [0, 1] or NaN. */
#define SILO_GPU_MAX_COMPARISON_TABLES 64
#define SILO_GPU_COMPARE_THREADS 256
int silo_gpu_mutations_compare(
   int alphabet, const uint32_t* counts_dev, uint32_t n_tables, uint32_t n_positions, const uint8_t* reference_index_dev, double min_proportion,
   double min_difference, uint32_t capacity, uint32_t* out_dev, void* stream
);

/* ---- K18: each row's differences from the reference (MutationsPerSequence / AminoAcidMutationsPerSequence) ----
 * Takes no store (like K10 and K17): it starts from the characters that silo_gpu_reconstruct_sequences writes for every store
 * layout, chars_dev[r * positions + p], rows back to back without padding (so a row starts at any byte alignment), and the
 * reference as characters, reference_dev[p].  With "valid" as in K10 (nucleotide "-ACGT", amino acid "-ACDEFGHIKLMNPQRSTVWY*") and
 * the missing symbol 'N' / 'X', the CLASS of the cell (r, p) with c = chars_dev[r * positions + p] is
 *     MISSING       c is the missing symbol, whatever the reference holds at p
 *     AMBIGUOUS     c is any other byte that is not valid: ambiguity codes, lower case, 0x00, 0xFF
 *     SAME          c is valid and equals reference_dev[p]
 *     DELETION      c is valid, differs from reference_dev[p] and is '-'
 *     SUBSTITUTION  c is valid, differs from reference_dev[p] and is not '-' (a reference byte that is not valid differs from
 *                   every valid c)
 * and the cell EMITS exactly one record word (p << 9) | (close << 8) | byte iff
 *     its class is SUBSTITUTION or AMBIGUOUS                                                      byte = c, close = 0
 *     its class is DELETION or MISSING and p == 0 or the class of (r, p - 1) differs: a run start  byte = c, close = 0
 *     its class is SAME, p > 0 and the class of (r, p - 1) is DELETION or MISSING: a run's close   byte = 0, close = 1
 * A run that is followed by a substitution, an ambiguous cell or a run of the other kind has no close: the next record's position
 * ends it; a run that reaches the end of the row is ended by `positions`.  The left neighbour is always a cell of the SAME row:
 * the last cell of row r - 1, which lies directly in front of (r, 0) in memory, is never looked at.
 * WRITES
 *     offsets_dev[0 .. n_rows]     offsets_dev[0] = 0, offsets_dev[r + 1] = the words of rows 0 .. r; offsets_dev[n_rows] may
 *                                  exceed `capacity`
 *     stats_dev[r * 4 + 0 .. 3]    the substitution, deleted, missing and ambiguous CELLS (not runs) of row r
 *     records_dev[i]               for i < min(offsets_dev[n_rows], capacity): word i of the ONE list of all rows' words, ordered by
 *                                  row, then by ascending position — with a short capacity an exact prefix; nothing at or past
 *                                  min(total, capacity) is touched.  capacity == 0 is legal (records_dev may then be NULL): the
 *                                  counts alone.
 * Every word of offsets_dev and stats_dev is written and nothing is accumulated into memory the caller would have to clear: a
 * second call gives the same bytes everywhere.  scratch_dev: SILO_GPU_DIFFERENCES_SCRATCH_BYTES(n_rows, positions) bytes, 4-byte
 * aligned like the three outputs — per (row, chunk) the words and the four cell counts; a chunk is the cells of a row in
 * SILO_GPU_DIFFERENCE_CHUNK bytes of memory counted from the 16-byte boundary at or below the row's first byte, so every chunk is
 * read with aligned 16-byte loads and a row has at most SILO_GPU_DIFFERENCE_CHUNKS(positions) of them.
 * Four launches on `stream`, no waiting, no atomics, no floating point: a count pass over (chunk, row) blocks (a thread per 16
 * bytes; the class left of a thread's first cell comes from the lane before, for a wave's first lane from one extra byte of the
 * same row); a wave per row that sums the row's chunks and turns their counts into starts within the row; one block that turns
 * the rows' totals into offsets_dev; a write pass that recomputes the flags and places each word at its chunk's start plus its
 * rank, every index checked against `capacity` (not launched for capacity == 0).  n_rows == 0 or positions == 0: success, the
 * offsets and stats written as 0, nothing launched.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an alphabet
 * other than the two, a NULL pointer (records_dev only where capacity != 0), a pointer that is not 4-byte aligned, n_rows >
 * SILO_GPU_MAX_DIFFERENCE_ROWS, positions > SILO_GPU_MAX_DIFFERENCE_POSITIONS or n_rows * positions >= 2^32. */
#define SILO_GPU_MAX_DIFFERENCE_ROWS 10000
#define SILO_GPU_MAX_DIFFERENCE_POSITIONS (1u << 23)
#define SILO_GPU_DIFFERENCE_STATS 4
#define SILO_GPU_DIFFERENCE_CHUNK 4096 /* bytes of a row per block: 256 threads x 16 bytes */
#define SILO_GPU_DIFFERENCE_CHUNKS(positions) (((positions) + 15u + SILO_GPU_DIFFERENCE_CHUNK - 1u) / SILO_GPU_DIFFERENCE_CHUNK)
#define SILO_GPU_DIFFERENCES_SCRATCH_BYTES(n_rows, positions) \
   ((size_t)(n_rows) * SILO_GPU_DIFFERENCE_CHUNKS(positions) * (1u + SILO_GPU_DIFFERENCE_STATS) * sizeof(uint32_t))
int silo_gpu_sequence_differences(
   int alphabet, const char* chars_dev /* [n_rows][positions] */, uint32_t n_rows, uint32_t positions, const char* reference_dev /* [positions] */,
   uint32_t capacity, uint32_t* offsets_dev /* n_rows + 1 */, uint32_t* stats_dev /* n_rows * 4 */,
   uint32_t* records_dev /* capacity words; may be NULL iff capacity == 0 */, void* scratch_dev, void* stream
);

/* ---- K11: the rows of the whole store nearest to a query (NearestNeighbours) --------------------------
 * silo_gpu_query_distances compares one query — query_chars, `positions` characters in HOST memory — with EVERY row of a sequence
 * store, read off the store's own layout (identity / code planes with escape keys, one-hot rows with a derived symbol, runs of the
 * missing symbol, sparse or extra ambiguity planes) instead of gathered characters.  It WRITES for every row r < row_words * 64
 *     out_dev[r * 2]     = distance = positions where the query and row r both hold a valid mutation symbol and the two differ
 *     out_dev[r * 2 + 1] = compared = positions where both hold a valid mutation symbol
 * with "valid" as in K10 (nucleotide "-ACGT", amino acid "-ACDEFGHIKLMNPQRSTVWY*"; every other byte of the query never compares):
 * exactly the two numbers silo_gpu_distance_pairs gives for the pair (query, r).  Rows at or past sequence_count get (0, 0); the
 * caller never clears out_dev.  Integer adds only: the table does not depend on how the blocks are scheduled.
 * scratch_dev: device memory of SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES(positions) bytes, 16-byte aligned.  Uploads its per-position
 * tables there and waits for them (one stream synchronisation), then launches its passes on `stream` without waiting: the constants
 * of the derived positions, the plane rows (a thread owns 64 rows and adds each position's masks into vertical counters of
 * SILO_GPU_QUERY_DISTANCE_COUNTER_PLANES bit planes), the escape keys, the runs of the missing symbol, the sparse keys.
 * silo_gpu_nearest_rows takes such a table (no store, like silo_gpu_mutations_select and K10) and WRITES the k smallest rows by
 * (distance, row) among the rows r < sequence_count that filter_dev selects (NULL = all rows; bits at or past sequence_count never
 * select a row), other than exclude_row (UINT32_MAX: none), with distance <= max_distance (UINT32_MAX: no bound):
 *     out_dev[i * 3 + 0 .. 2] = row, distance, compared     for i < *out_count_dev <= k, ascending by (distance, row)
 * Entries at or past *out_count_dev are not touched.  Rows tied at the k-th distance are taken by ascending row id; two calls with
 * the same arguments give the same output.  scratch_dev: SILO_GPU_NEAREST_ROWS_SCRATCH_BYTES bytes, 16-byte aligned.  Launches on
 * `stream` and returns without waiting.
 * Both fail with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL store, query, table, output or scratch, a seqstore_id
 * out of range, a store or table without rows, k == 0 or k > SILO_GPU_MAX_NEAREST_ROWS.
 * silo_gpu_bitset_from_distances takes such a table of row_words * 64 rows (no store either) and WRITES every one of the row_words
 * words of out_bitset_dev — the caller never clears it, nothing past row_words is touched:
 *     bit r = r < sequence_count && distance[r] <= max_distance && compared[r] >= min_compared
 * max_distance == UINT32_MAX: no bound on the distance; min_compared == 0: none on the compared positions.  Rows at or past
 * sequence_count are 0 whatever the table holds there (the filter kernels and the derived-symbol count rely on clean padding).
 * This is the leaf of the filter expression WithinDistance: the 8 bytes per row of the table never leave the device.  One launch
 * on `stream` (a thread per row, one 8-byte load each, a wave's ballot is a word; no atomics: the same arguments give the same
 * words), returns without waiting.  Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL table or output,
 * row_words == 0, sequence_count == 0 or sequence_count > row_words * 64. */
#define SILO_GPU_MAX_NEAREST_ROWS 1024
#define SILO_GPU_QUERY_DISTANCE_COUNTER_PLANES 12 /* a vertical counter is unpacked after 2^12 - 1 adds */
#define SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES(positions)                                                                    \
   (((size_t)(positions) / 256u + 1u) * 256u + 2u * ((((size_t)(positions) + 1u) * 4u) / 256u + 1u) * 256u)
#define SILO_GPU_NEAREST_ROWS_SCRATCH_BYTES 32768u
int silo_gpu_query_distances(
   const silo_gpu_store* store, uint32_t seqstore_id, const char* query_chars, uint32_t* out_dev, void* scratch_dev, void* stream
);
int silo_gpu_nearest_rows(
   const uint32_t* table_dev, const uint64_t* filter_dev, uint32_t sequence_count, uint32_t exclude_row, uint32_t max_distance, uint32_t k,
   uint32_t* out_dev, uint32_t* out_count_dev, void* scratch_dev, void* stream
);
int silo_gpu_bitset_from_distances(
   const uint32_t* table_dev, uint32_t sequence_count, uint32_t row_words, uint32_t max_distance, uint32_t min_compared, uint64_t* out_bitset_dev,
   void* stream
);

/* ---- K19: a seeded random subset of a filter's rows (the filter expression Sample) -----------------------
 * Row r of a partition whose first row has the number first_row in the database is the GLOBAL row first_row + r (< 2^32), and
 *     key(seed, row) = fmix32(fmix32(row + k1) ^ k2)   with k1 / k2 = the low / high 32 bits of splitmix64(seed)
 * (fmix32: MurmurHash3's finaliser; arithmetic mod 2^32, splitmix64 mod 2^64) — a bijection of uint32, so no two rows tie.
 * silo_gpu_sample_key is that function on the host; the kernels compile the same code.  The entries take no store (like
 * silo_gpu_nearest_rows and silo_gpu_bitset_from_distances).  A selection of the `size` smallest keys per group ("stratum") of rows,
 * over any number of partitions, is a radix select in four rounds of 8 key bits, most significant first, all on the device:
 *     silo_gpu_sample_begin, then for round = 0 .. 3 { silo_gpu_sample_count per partition; silo_gpu_sample_advance },
 *     then silo_gpu_sample_select per partition.
 * groups_dev: uint16 [row_words * 64], a row's group (< n_groups) or 0xFFFF (any value >= n_groups) for none; NULL = one group that
 * holds every selected row.  A row COUNTS when its bit in filter_dev is set, it is < sequence_count (padding bits of a filter never
 * select a row) and it has a group.
 * state_dev: SILO_GPU_SAMPLE_STATE_BYTES(n_groups) bytes, 16-byte aligned, as uint32 words
 *     [0] n_groups  [1] size  [2] k1  [3] k2
 *     [4 + 4g + 0 .. 2]  per group g: the key prefix found so far, the rows still to take under that prefix, the take-all flag
 *     [4 + 4 * n_groups + g * 256 + d]  the round's histogram
 * silo_gpu_sample_groups WRITES groups_out_dev[r] for every r < row_words * 64: the date range (index into range_bounds, the ranges
 *     and the rules for them exactly as for K7: both ends inclusive, 0 / 0xFFFFFFFF where unbounded, pairwise disjoint, NULL dates
 *     in no range) of each counting row, 0xFFFF for every other row.  Uploads the sorted ranges and waits for the stream once, behind
 *     its launch.
 * silo_gpu_sample_begin WRITES the whole state: no prefix, `size` rows to take in every group, histogram 0.  1 <= n_groups <=
 *     SILO_GPU_MAX_SAMPLE_GROUPS.
 * silo_gpu_sample_count adds 1 to the histogram cell [group][digit] for every counting row whose group is not take-all and whose
 *     key's top 8 * round bits equal the group's prefix; digit = the next 8 key bits.  ACCUMULATED, like K1, K7, K8 and K9: one call
 *     per partition fills one table, which is what makes the selection global.  Integer adds only: the table does not depend on how
 *     the blocks are scheduled.  Up to SILO_GPU_SAMPLE_LDS_GROUPS groups a block counts into a histogram in LDS and adds its
 *     non-zero cells to the table; above, every row adds to the table directly.
 * silo_gpu_sample_advance, per group that is not take-all: in round 0 a group whose histogram sums to <= size becomes take-all;
 *     otherwise the first digit whose running sum reaches the rows still to take is appended to the prefix and the cells in front
 *     of it are subtracted from the rows still to take.  Clears the histogram.  After round 3 the prefix is the largest selected
 *     key of the group and exactly one row is still to take.
 * silo_gpu_sample_select WRITES every one of the row_words words of out_bitset_dev and nothing behind them:
 *     bit r = r counts && (take_all[group] || key(r) <= prefix[group]), and 0 for every r when size == 0.
 * All launch on `stream` and return without waiting (silo_gpu_sample_groups: see above).  Each fails with
 * SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL state, filter, date column, ranges or output, row_words == 0,
 * sequence_count > row_words * 64, n_groups / n_ranges outside 1 .. 1 024, ranges K7 refuses, size > INT32_MAX, round > 3, or
 * first_row + sequence_count > 2^32. */
#define SILO_GPU_MAX_SAMPLE_GROUPS 1024
#define SILO_GPU_SAMPLE_LDS_GROUPS 16 /* 16 x 256 cells of 4 bytes: 16 KiB of a block's LDS */
#define SILO_GPU_SAMPLE_ROUNDS 4
#define SILO_GPU_SAMPLE_STATE_BYTES(n_groups) (16u + (size_t)(n_groups) * (16u + 256u * 4u))
uint32_t silo_gpu_sample_key(uint64_t seed, uint32_t global_row);
int silo_gpu_sample_groups(
   const uint64_t* filter_dev, const uint32_t* date_column_dev, const uint32_t* range_bounds, uint32_t n_ranges, uint32_t sequence_count,
   uint32_t row_words, uint16_t* groups_out_dev, void* stream
);
int silo_gpu_sample_begin(void* state_dev, uint32_t n_groups, uint32_t size, uint64_t seed, void* stream);
int silo_gpu_sample_count(
   void* state_dev, const uint64_t* filter_dev, const uint16_t* groups_dev, uint32_t sequence_count, uint32_t row_words, uint32_t first_row,
   uint32_t round, void* stream
);
int silo_gpu_sample_advance(void* state_dev, uint32_t round, void* stream);
int silo_gpu_sample_select(
   const void* state_dev, const uint64_t* filter_dev, const uint16_t* groups_dev, uint32_t sequence_count, uint32_t row_words,
   uint32_t first_row, uint64_t* out_bitset_dev, void* stream
);

/* ---- K20: one row per distinct aligned sequence (the filter expression DistinctSequences) -----------------
 * sym(r, p) is the index of the symbol row r holds at position p in the alphabet's own order — what silo_gpu_reconstruct_sequences
 * turns into a character — and 31 for a cell that nothing stored claims (its '?').  With splitmix64 as in K19, mod 2^64:
 *     x = p * 32 + sym,   H0(p, sym) = splitmix64(x),   H1(p, sym) = splitmix64(x + 2^40)
 *     hash(r) = (sum over p of H0(p, sym(r, p)), sum over p of H1(p, sym(r, p)))
 * Rows with equal aligned sequences have equal hashes; rows with equal hashes are TREATED as equal (two given different rows
 * collide with probability 2^-128 for a function drawn at random): the one probabilistic answer of this library.
 * silo_gpu_row_hash_term is H0 (lane 0) / H1 (lane 1) on the host; the kernels compile the same code.
 * silo_gpu_row_hashes WRITES out_dev[r] = hash(r) for every r < sequence_count and (0, 0) for every other r < row_words * 64, for a
 *     finalized store in any layout: the plane pass writes each row's sums over what the planes say (code planes, one-hot rows,
 *     extra planes; a cell they leave open counts as the position's derived symbol, or as 31 where none is derived) with plain
 *     16-byte stores, then a thread per escape key, per run of the missing symbol and per sparse key adds the difference between its
 *     symbol's term and the one the plane pass assumed (64-bit integer atomics: exact, whatever the schedule).  scratch_dev:
 *     SILO_GPU_ROW_HASH_SCRATCH_BYTES(positions) bytes, 256-byte aligned, for two per-position tables built on the host; uploads
 *     them and waits for the stream once, ahead of its launches.
 * silo_gpu_store_row_hashes returns the store's own copy of that table: the first call per sequence store allocates 16 bytes x
 *     row_words * 64 (from then on part of silo_gpu_store_device_bytes), runs silo_gpu_row_hashes on `stream` and waits; every
 *     later call returns the same pointer without device work.  Thread-safe.  The table lives as long as the store.
 * Both fail with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, a seqstore_id out of range or a store that is
 * not finalized.
 *
 * The selection takes no store.  A database is an array of PARTS ordered by first_row; row r of a part is the GLOBAL row
 * first_row + r (< 2^32 - 1).  table_dev: SILO_GPU_DISTINCT_TABLE_BYTES(slots) bytes as uint32 — `slots` owners (a power of two; the
 * global row that represents a class, 0xFFFFFFFF = empty) and one overflow counter behind them.
 * silo_gpu_distinct_begin WRITES the whole table: every slot empty, the counter 0.
 * silo_gpu_distinct_insert, once per part: every row of the part that counts — its bit in filter_dev set and r < sequence_count
 *     (padding bits of a filter never select a row) — probes linearly from (lane 0 of its hash) & (slots - 1): an empty slot is
 *     claimed with a compare-and-swap; a slot whose owner has the row's hash takes the smaller of the two global rows (atomic min);
 *     any other slot is passed.  A slot, once claimed, only ever holds rows of one class, and a class only ever sits in one slot.
 *     A row that has passed `slots` slots adds 1 to the overflow counter and gives up: with slots >= 2 x the rows inserted this
 *     does not happen.  After the inserts of all parts a class's slot holds its smallest global row, whatever the schedule.
 * silo_gpu_distinct_select WRITES every one of the part's row_words words of out_bitset_dev and nothing behind them:
 *     bit r = r counts && the slot of r's class is owned by first_row + r   (a read-only probe).
 * All launch on `stream`.  silo_gpu_distinct_begin returns without waiting; insert and select read parts_dev[part] back first (24
 * bytes behind whatever `stream` holds: one wait ahead of the launch), which sizes the grid and is what they check.  Each fails with
 * SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, slots 0 or not a power of two, n_parts == 0, part >= n_parts,
 * a part with a NULL hash table, row_words == 0, sequence_count > row_words * 64 or first_row + sequence_count >= 2^32 - 1. */
#define SILO_GPU_ROW_HASH_NO_SYMBOL 31u
#define SILO_GPU_ROW_HASH_SCRATCH_BYTES(positions) ((size_t)(positions) * 17u + 1024u)
#define SILO_GPU_DISTINCT_EMPTY 0xFFFFFFFFu
#define SILO_GPU_DISTINCT_TABLE_BYTES(slots) (((size_t)(slots) + 1u) * 4u)
typedef struct silo_gpu_distinct_part {
   const uint64_t* hashes_dev; /* [row_words * 64][2], as silo_gpu_row_hashes writes them */
   uint32_t first_row;
   uint32_t sequence_count;
   uint32_t row_words;
   uint32_t reserved;
} silo_gpu_distinct_part;
uint64_t silo_gpu_row_hash_term(uint32_t position, uint32_t symbol, uint32_t lane);
int silo_gpu_row_hashes(const silo_gpu_store* store, uint32_t seqstore_id, uint64_t* out_dev, void* scratch_dev, void* stream);
int silo_gpu_store_row_hashes(silo_gpu_store* store, uint32_t seqstore_id, const uint64_t** out_dev, void* stream);
int silo_gpu_distinct_begin(void* table_dev, uint32_t slots, void* stream);
int silo_gpu_distinct_insert(
   void* table_dev, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part, const uint64_t* filter_dev,
   void* stream
);
int silo_gpu_distinct_select(
   const void* table_dev, uint32_t slots, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, uint64_t* out_bitset_dev, void* stream
);

/* ---- K21: the sizes of a selection's sequence classes (the action DistinctSequenceCounts) -----------------
 * On a table that silo_gpu_distinct_begin and EVERY part's silo_gpu_distinct_insert have filled, with the same slots, parts and
 * filters as those calls.  A row COUNTS as for K20.  The slot of a counting row's class is where the read-only probe of
 * silo_gpu_distinct_select ends: at the slot the row owns, or at the first slot whose owner has the row's hash.
 * silo_gpu_distinct_count, once per part after every part's insert: adds to counts_dev[slot] (uint32 [slots],
 *     SILO_GPU_DISTINCT_COUNTS_BYTES(slots) bytes, cleared by the caller) the part's counting rows whose class sits in `slot`.
 *     ACCUMULATED over the parts, like K19's histogram: after the calls of all parts counts_dev[slot] is the size of the class that
 *     owns `slot` and 0 for every other slot.  A wave adds once per distinct slot among its 64 rows (the first lane's slot, a ballot
 *     of the lanes that share it) for a bounded number of rounds, then once per row: integer adds only, so the counts depend neither
 *     on that bound nor on the schedule.  A counting row whose probe finds neither itself nor its class — there is none after the
 *     inserts — adds 1 to the table's overflow counter and to nothing else.  Writes nothing else of the table.
 * silo_gpu_distinct_classes, once per part after every part's count: every counting row that OWNS its slot and whose
 *     counts_dev[slot] >= min_count appends the key  (uint64)(0xFFFFFFFF - count) << 32 | global row  to keys_dev — ascending keys are
 *     descending counts, then ascending representatives.  Appends ACCUMULATE over the parts from *n_keys_dev, which the caller
 *     clears: one atomic add per wave and step of 16 filter words.  Nothing is written at or past keys_dev[capacity], but *n_keys_dev counts every class that
 *     qualifies, so a caller sees a list that was too short.  The order of keys_dev is unspecified, its set is not.
 * silo_gpu_smallest_keys takes no table: of the n = min(*n_keys_dev, capacity) keys of keys_dev, which have to be PAIRWISE DISTINCT,
 *     it WRITES the k smallest (all n if n <= k) to out_dev in unspecified order and *out_count_dev = min(n, k); entries of out_dev
 *     at or past that count are untouched.  n is read on the device.  A radix select as K19's with one group: eight rounds of 8 key
 *     bits, most significant first, each a histogram launch (a block's 256 cells in LDS, its non-zero cells added to the table) and
 *     a one-block launch that fixes the digit; then one launch that appends every key <= the k-th smallest.  With equal keys more
 *     than k may qualify: never more than k entries are written, which of them is then unspecified.  scratch_dev:
 *     SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES bytes, 8-byte aligned; the call clears it.
 * All launch on `stream`; count and classes read parts_dev[part] back first, as insert and select do, and nothing else returns to
 * the host.  Each fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for whatever insert and select refuse, a NULL pointer,
 * capacity == 0, min_count == 0, k == 0 or k > SILO_GPU_MAX_DISTINCT_CLASSES. */
#define SILO_GPU_MAX_DISTINCT_CLASSES 16384
#define SILO_GPU_DISTINCT_COUNTS_BYTES(slots) ((size_t)(slots) * 4u)
#define SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES 1088u /* 256 histogram cells and 16 words of state */
int silo_gpu_distinct_count(
   void* table_dev, uint32_t slots, uint32_t* counts_dev, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, void* stream
);
int silo_gpu_distinct_classes(
   void* table_dev, uint32_t slots, const uint32_t* counts_dev, const silo_gpu_distinct_part* parts_dev, uint32_t n_parts, uint32_t part,
   const uint64_t* filter_dev, uint32_t min_count, uint64_t* keys_dev, uint32_t capacity, uint32_t* n_keys_dev, void* stream
);
int silo_gpu_smallest_keys(
   const uint64_t* keys_dev, const uint32_t* n_keys_dev, uint32_t capacity, uint32_t k, uint64_t* out_dev, uint32_t* out_count_dev, void* scratch_dev,
   void* stream
);

/* ---- K22: each row's cell counts, kept by the store (the filter expression CellCount, the action CellCountDistribution) ----
 * The class of the cell of row r at position p is K18's, word for word, with sym(r, p) as for K20 and ref[p] the sequence store's own
 * reference: MISSING where sym is the missing symbol (N / X) whatever the reference holds; AMBIGUOUS where it is any other symbol
 * that is no valid mutation symbol, or 31; SAME where it is valid and equals ref[p]; DELETION where it is valid, differs and is '-';
 * SUBSTITUTION otherwise.  A reference symbol that is not valid differs from every valid symbol.  cells(r) is four uint32 in the
 * order of K18's stats — substitutions, deletions, missing, ambiguous — over ALL positions: what silo_gpu_sequence_differences
 * reports for the characters silo_gpu_reconstruct_sequences gives for row r.
 * silo_gpu_row_cell_counts WRITES out_dev[r] = cells(r) for every r < sequence_count and (0, 0, 0, 0) for every other
 *     r < row_words * 64, for a finalized store in any layout, as silo_gpu_row_hashes writes its hashes: the plane pass stores each
 *     row's counts over what the planes say (an open cell counts as the position's derived symbol, or as 31), then a thread per
 *     escape key, per run of the missing symbol and per sparse key adds the difference between its symbol's class and the one the
 *     plane pass assumed (32-bit integer atomics: exact, whatever the schedule).  scratch_dev:
 *     SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(positions) bytes, 256-byte aligned, for two per-position tables built on the host;
 *     uploads them and waits for the stream once, ahead of its launches.
 * silo_gpu_store_row_cell_counts returns the store's own copy of that table: the first call per sequence store allocates 16 bytes x
 *     row_words * 64 (from then on part of silo_gpu_store_device_bytes), runs silo_gpu_row_cell_counts on `stream` and waits; every
 *     later call returns the same pointer without device work.  Thread-safe.  The table lives as long as the store.
 * Both fail with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, a seqstore_id out of range or a store that is
 * not finalized.
 *
 * The two readers take no store, only such a table (16-byte aligned).  value(r) is the sum of the counts of row r whose bit is set
 * in kinds_mask (bit k = entry k of cells(r)), a 64-bit sum.
 * silo_gpu_bitset_from_cell_counts WRITES every one of the row_words words of out_bitset_dev and nothing behind them:
 *     bit r = r < sequence_count && at_least <= value(r) <= at_most   (at_least > at_most selects nothing).
 * silo_gpu_cell_count_histogram ADDS to bins_dev[min(value(r) / bin_width, n_bins - 1)] (uint64 [n_bins], cleared by the caller;
 *     partitions accumulate into one array) one for every row r < sequence_count whose bit in filter_dev is set (NULL: every row;
 *     padding bits never count).  A block counts in LDS and adds its non-zero cells to bins_dev with 64-bit integer atomics.
 * Both launch on `stream` and return without waiting.  Each fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL
 * table or output, row_words == 0, sequence_count == 0 or > row_words * 64, kinds_mask == 0 or > 15; the histogram also for
 * bin_width == 0, n_bins == 0 or n_bins > SILO_GPU_MAX_CELL_COUNT_BINS. */
#define SILO_GPU_CELL_COUNT_KINDS 4
#define SILO_GPU_CELL_COUNT_SUBSTITUTIONS 1u
#define SILO_GPU_CELL_COUNT_DELETIONS 2u
#define SILO_GPU_CELL_COUNT_MISSING 4u
#define SILO_GPU_CELL_COUNT_AMBIGUOUS 8u
#define SILO_GPU_MAX_CELL_COUNT_BINS 4096
#define SILO_GPU_ROW_CELL_COUNT_SCRATCH_BYTES(positions) ((size_t)(positions) * 17u + 1024u)
int silo_gpu_row_cell_counts(const silo_gpu_store* store, uint32_t seqstore_id, uint32_t* out_dev, void* scratch_dev, void* stream);
int silo_gpu_store_row_cell_counts(silo_gpu_store* store, uint32_t seqstore_id, const uint32_t** out_dev, void* stream);
int silo_gpu_bitset_from_cell_counts(
   const uint32_t* table_dev, uint32_t row_words, uint32_t sequence_count, uint32_t kinds_mask, uint32_t at_least, uint32_t at_most,
   uint64_t* out_bitset_dev, void* stream
);
int silo_gpu_cell_count_histogram(
   const uint32_t* table_dev, uint32_t row_words, uint32_t sequence_count, const uint64_t* filter_dev, uint32_t kinds_mask, uint32_t bin_width,
   uint32_t n_bins, uint64_t* bins_dev, void* stream
);

/* ---- K23: cell counts over position ranges (the filter expression CellCount with positionFrom / positionTo, the action
 * CellCountByRegion) ----
 * A region is a range [first, end) of 0-based positions of one sequence store.  value(r, g) is the number of positions p of region g
 * whose cell of row r has a class (K22's, word for word) whose bit is set in kinds_mask; for the region [0, positions) it is K22's
 * value(r).  Nothing is kept by the store.
 * silo_gpu_region_cell_values WRITES values_dev[g * row_words * 64 + r] = value(r, g) for every r < sequence_count and 0 for every
 *     other r < row_words * 64, for each of the n_ranges regions of `ranges` (HOST memory, uint32 [n_ranges][2] = first, end; read
 *     before the call returns), for a finalized store in any layout: region g's column is a plain array of 4 bytes per row.  The
 *     ranges are ascending, pairwise disjoint and non-empty, end <= positions.  It is K22's decomposition with a 0/1 weight in place
 *     of a class vector: a plane pass with a wave per (row word, region) that walks the region's positions only and stores the
 *     value once; then a thread per escape key and per sparse key of the ranges' slices of the position-major key lists (the
 *     slices of all ranges flattened into one index space: one launch each), and a thread per run of the missing symbol that
 *     visits the regions the run meets with two lookups in a prefix array each — all adding the difference between the weight of
 *     their symbol and the one the plane pass assumed (32-bit integer atomics: exact, whatever the schedule).  scratch_dev:
 *     SILO_GPU_REGION_VALUE_SCRATCH_BYTES(positions) bytes, 256-byte aligned, for per-position and per-range tables built on the
 *     host; uploads them and waits for the stream once, ahead of its launches.
 *     Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, a seqstore_id out of range, a store that is not
 *     finalized, n_ranges == 0 or > SILO_GPU_MAX_REGIONS, a range that is empty, out of order, overlapping or past the end,
 *     kinds_mask == 0 or > 15.
 * The two readers take no store, only columns of such values.
 * silo_gpu_bitset_from_values WRITES every one of the row_words words of out_bitset_dev and nothing behind them, from ONE column:
 *     bit r = r < sequence_count && at_least <= values_dev[r] <= at_most   (at_least > at_most selects nothing).
 * silo_gpu_count_values ADDS to counts_dev[c] (uint64 [n_columns], cleared by the caller; partitions and chunks accumulate), for
 *     each of the n_columns columns of values_dev (uint32 [n_columns][row_words * 64]), the number of rows r < sequence_count whose
 *     bit in filter_dev is set (NULL: every row; padding bits never count) and bounds[c][0] <= values_dev[c][r] <= bounds[c][1]
 *     (`bounds`: HOST memory, uint32 [n_columns][2], passed on as kernel arguments).  A block sums its waves' popcounts and adds a
 *     non-zero sum with one 64-bit integer atomic per column.  n_columns is 1 .. SILO_GPU_MAX_REGIONS.
 * Both launch on `stream` and return without waiting.  Each fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for a NULL
 * values, output or bounds pointer, row_words == 0, sequence_count == 0 or > row_words * 64; the count also for n_columns == 0 or
 * > SILO_GPU_MAX_REGIONS. */
#define SILO_GPU_MAX_REGIONS 256
#define SILO_GPU_REGION_VALUE_SCRATCH_BYTES(positions) ((size_t)(positions) * 7u + 8192u)
int silo_gpu_region_cell_values(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint32_t* ranges, uint32_t n_ranges, uint32_t kinds_mask, uint32_t* values_dev,
   void* scratch_dev, void* stream
);
int silo_gpu_bitset_from_values(
   const uint32_t* values_dev, uint32_t row_words, uint32_t sequence_count, uint32_t at_least, uint32_t at_most, uint64_t* out_bitset_dev, void* stream
);
int silo_gpu_count_values(
   const uint32_t* values_dev, uint32_t n_columns, uint32_t row_words, uint32_t sequence_count, const uint64_t* filter_dev, const uint32_t* bounds,
   uint64_t* counts_dev, void* stream
);

/* ---- K24: pairwise sums of count tables (MeanDistances / AminoAcidMeanDistances) --------------------------
 * Takes no store.  counts_dev is as for silo_gpu_mutations_compare: 1 <= n_tables <= SILO_GPU_MAX_PAIR_SUM_TABLES tables back to
 * back, n_positions x n_symbols words each (n_symbols = 5 / 22), 4-byte aligned.  `ranges` (HOST memory, uint32 [n_ranges][2] =
 * first, end, 0-based; read before the call returns): 1 <= n_ranges <= SILO_GPU_MAX_PAIR_SUM_RANGES ranges of positions, each
 * non-empty with end <= n_positions, in any order; they may overlap.  With c[t][p][s] a cell and cov[t][p] = sum_s c[t][p][s] (a
 * uint32: no wrap is defined), WRITES out_dev: for every range r and every pair of tables g <= h, in the order r, g, h, one record
 * of SILO_GPU_PAIR_SUM_WORDS uint64 words, n_ranges * G (G + 1) / 2 records for G = n_tables, 8-byte aligned:
 *     {diff_lo, diff_hi}   the 128-bit sum over the positions p of the range of
 *                              g < h    cov[g][p] * cov[h][p] - sum_s c[g][p][s] * c[h][p][s]
 *                              g == h   (cov[g][p]^2 - sum_s c[g][p][s]^2) / 2 (an integer: the unordered pairs of rows that differ)
 *     {cmp_lo, cmp_hi}     the 128-bit sum of cov[g][p] * cov[h][p] for g < h, of cov[g][p] * (cov[g][p] - 1) / 2 for g == h
 *     sites                g == h   the positions of the range where at least two symbols have a count above 0 (segregating sites)
 *                          g < h    the positions where cov[g][p] * cov[h][p] > 0 and sum_s c[g][p][s] * c[h][p][s] == 0 (fixed
 *                                   differences: both tables covered, no symbol in both)
 * They are the sums, over every pair of a row of g and a row of h (for g == h: every unordered pair of two rows), of K10's
 * `distance` and `compared` of the pair restricted to the range, when the tables are exact Mutations tables of the rows.
 * Integers only.  A position's term fits 64 bits; a thread carries the high word of its sums itself and a block adds what it has
 * with 64-bit integer atomics, one more on the high word where its add on the low word wrapped: exact, whatever the schedule.  The
 * entry clears the records itself, on `stream`, so a second call gives the same bytes; the caller clears nothing.  One kernel
 * launch: a block of 256 threads owns a tile of SILO_GPU_PAIR_SUM_TILE x SILO_GPU_PAIR_SUM_TILE pairs of the upper triangle and up to
 * SILO_GPU_PAIR_SUM_CHUNK positions of one range, which it stages through LDS SILO_GPU_PAIR_SUM_POSITION_TILE positions at a time; the
 * jobs (range, chunk, tile of pairs) of all ranges are one grid.  Returns without waiting.
 * Fails with SILO_GPU_ERR_INVALID_ARGUMENT, nothing written, for an alphabet other than the two, a NULL pointer, tables that are not
 * 4-byte or records that are not 8-byte aligned, n_tables == 0 or above the limit, n_ranges == 0 or above the limit, n_positions ==
 * 0, a range that is empty or ends past n_positions, or more jobs than a grid holds (2^31 - 1). */
#define SILO_GPU_MAX_PAIR_SUM_TABLES 64
#define SILO_GPU_MAX_PAIR_SUM_RANGES 256
#define SILO_GPU_PAIR_SUM_WORDS 5
#define SILO_GPU_PAIR_SUM_TILE 16
#define SILO_GPU_PAIR_SUM_POSITION_TILE 16
#define SILO_GPU_PAIR_SUM_CHUNK 128
int silo_gpu_table_pair_sums(
   int alphabet, const uint32_t* counts_dev, uint32_t n_tables, uint32_t n_positions, const uint32_t* ranges, uint32_t n_ranges, uint64_t* out_dev,
   void* stream
);

/* The same scan for a batch of filters over one sequence store: every plane row is read once for up to
 * SILO_GPU_MAX_SCAN_BATCH filters per pass (larger batches take several passes), counts_out_dev[q] is
 * accumulated with filters_dev[q].  This is how concurrent Mutations queries share the HBM stream. */
enum { SILO_GPU_MAX_SCAN_BATCH = 8 };
int silo_gpu_mutations_scan_batch(
   const silo_gpu_store* store, uint32_t seqstore_id, const uint64_t* const* filters_dev, uint32_t n_filters,
   uint32_t pos_begin, uint32_t pos_end, uint32_t* const* counts_out_dev, void* stream
);
int silo_gpu_memset_async(void* dev_ptr, int value, size_t bytes, void* stream);

/* Tuning knobs of K1 (0 = default); returns the previous value.  For benchmarks only. */
enum { SILO_GPU_TUNE_SCAN_ROWS_PER_BLOCK = 0, SILO_GPU_TUNE_SCAN_VARIANT = 1, SILO_GPU_TUNE_EVAL_LEAF_BATCH = 2 /* 8 (default) or 16 leaf loads in flight per lane in K3 */,
       SILO_GPU_TUNE_COMPACT_INDEX = 4 /* finalize: < 0 keeps the build-time identity planes, 0 (default) re-encodes every position into its cheapest
                                          layout (one-hot rows with the most numerous symbol derived, 2 / 3 code planes, identity planes), 2 the same
                                          without one-hot rows, 3 with a one-hot row for the most numerous symbol too (nothing derived) */,
       SILO_GPU_TUNE_KEY_COST = 6 /* finalize: > 0 = the cost of an escape key, in plane bytes, in the choice of layouts (experiments) */,
       SILO_GPU_TUNE_MISSING_RUNS = 8 /* finalize: < 0 keeps the plane of the missing symbol (N / X) instead of turning it into runs */,
       SILO_GPU_TUNE_LAUNCH_COST = 9 /* finalize: what a further kind of plane-scan launch costs in the choice of layouts, in KiB of plane bytes; 0 = default (192 MiB), < 0 = nothing (small test stores that are to mix layouts) */,
       SILO_GPU_TUNE_SCAN_TIMING = 7 /* 1: bracket every plane-scan launch with HIP events (silo_gpu_scan_timings) */,
       SILO_GPU_TUNE_SIDE_STREAM = 5 /* the escape-key pass of a scan: 0 (default) on a side stream of the lowest priority, 1 of default priority, 2 on the caller's stream, 3 = as 0 over the position-major keys (k_scan_escapes) */,
       SILO_GPU_TUNE_GAP_EVENTS = 10 /* a scan over a store with derived symbols: 0 (default) counts the rows without a valid symbol from the store's gap
                                        events in the escape-key pass (k_scan_escapes_sliced); < 0 takes the runs of the missing symbol and the sparse
                                        keys by themselves (k_scan_missing_runs, k_sum_run_parts, k_count_sparse_keys on a side stream), as SILO_GPU_TUNE_SIDE_STREAM = 3
                                        and stores of more than 67 M rows always do */,
       SILO_GPU_TUNE_PRUNE_KEYS = 11 /* silo_gpu_mutations_scan_ranges_min_proportion: 0 (default) skips the granules of escape keys and the one-hot
                                        plane rows that cannot reach a filter's proportion; 1 skips keys only; < 0 skips nothing (the exact scan) — for A/B runs */,
       SILO_GPU_TUNE_END_RUNS = 12 /* a Mutations scan over a store with end runs of the gap symbol (silo_gpu_store_scan_covered_rows): 0 (default) counts
                                      the covered one-hot rows of '-' from the sequences' end events and residual keys in the escape-key pass; 1 counts
                                      them in a launch of their own behind the row launch; < 0 reads the rows — the same tables either way, for A/B runs */,
       SILO_GPU_TUNE_FUSED_SELECT = 13 /* silo_gpu_mutations_scan_select: 0 (default) lets the finish kernel of the scan overwrite the tables and select the
                                          rows where the call allows it, < 0 always clears, scans and selects in launches of their own (comparisons) */,
       SILO_GPU_TUNE_ESCAPE_BLOCKS = 14 /* the blocks that walk the items — (range, slice, share) — of a sliced escape-key launch (k_scan_escapes_sliced):
                                           0 (default) one block per item, < 0 as many blocks as the chip holds at once, n > 0 exactly min(n, items)
                                           blocks, planned as for a chip of n places (tests) — the same tables whatever the value; one block per item
                                           is the faster on the headline (profiles/r10_escape_items.md), the others are kept for A/B runs */,
       SILO_GPU_TUNE_SCAN_SPARSE_DIVISOR = 3 /* a filter with a set bit in <= row_words / divisor of its 64-byte sectors takes the gather scan (K1s); 0 = default 16, < 0 = off */ };
int silo_gpu_tune(int knob, int value);

/* HIP events on the caller's stream, so a host without the HIP headers can time the kernels
 * (bench.py measures the roofline numbers with these, on the stream the kernels are launched on). */
int silo_gpu_event_create(void** out_event);
int silo_gpu_event_record(void* event, void* stream);
int silo_gpu_event_synchronize(void* event); /* blocks the calling thread until the event has happened */
int silo_gpu_event_elapsed_ms(void* start_event, void* stop_event, float* out_ms); /* synchronises on stop */
void silo_gpu_event_destroy(void* event);

/* ---- exchange step of the sharded scan: RCCL over xGMI -------------------------------------
 * One process per GPU.  The reference sums its partitions in a host loop inside one process (query_engine.cpp:40-49,
 * mutations.cpp:71,108); across GPUs that sum is ONE all-reduce of the count table per query (position-range or
 * sequence-id shards alike), and a filter leaf at a position another rank holds is ONE broadcast of a row bitset.
 * silo_gpu_comm_unique_id: called by one rank; the SILO_GPU_COMM_ID_BYTES opaque bytes reach the other ranks out
 * of band (the launcher's key-value store, MPI, a file).  silo_gpu_comm_create: collective over all `world` ranks.
 * The collectives are enqueued on `stream` (any stream of the communicator's device; NULL = the null stream) and
 * ordered with the kernels on it — no host synchronisation.  Every rank must enqueue the same collectives in the same
 * order; calls on one communicator are serialised internally.  librccl is bound on first use: without it these
 * fail with SILO_GPU_ERR_UNSUPPORTED and nothing else in the library is affected. */
typedef struct silo_gpu_comm silo_gpu_comm;
enum { SILO_GPU_COMM_ID_BYTES = 128 };
int silo_gpu_comm_unique_id(uint8_t* out_id /* [SILO_GPU_COMM_ID_BYTES] */);
int silo_gpu_comm_create(const uint8_t* id, uint32_t rank, uint32_t world, int device, silo_gpu_comm** out);
void silo_gpu_comm_destroy(silo_gpu_comm* comm);
uint32_t silo_gpu_comm_rank(const silo_gpu_comm* comm);
uint32_t silo_gpu_comm_world(const silo_gpu_comm* comm);
/* counts_dev[i] = sum over ranks of counts_dev[i], in place (ncclAllReduce, ncclUint32, ncclSum). */
int silo_gpu_allreduce_counts(silo_gpu_comm* comm, uint32_t* counts_dev, size_t n, void* stream);
/* bytes_dev of rank `root` to every rank, in place (ncclBroadcast). */
int silo_gpu_broadcast_bytes(silo_gpu_comm* comm, void* bytes_dev, size_t n_bytes, uint32_t root, void* stream);

/* Name of the last kernel variant silo_gpu_mutations_scan launched (for roofline attribution). */
const char* silo_gpu_last_scan_kernel(void);
/* Items — (range, slice, share) — of the calling thread's last launch of k_scan_escapes_sliced (0 before the first); the blocks that
 * walked them are the launch's `blocks` in the timing log (SILO_GPU_TUNE_ESCAPE_BLOCKS). */
uint32_t silo_gpu_last_escape_items(void);

/* Per-launch timing of a scan (measurement only).  With SILO_GPU_TUNE_SCAN_TIMING set to 1, every k_scan_sliced,
 * k_scan_escapes_sliced, k_scan_missing_runs and k_count_sparse_keys launch of the calling thread's scans is bracketed by HIP
 * events on the stream it is launched on; this call waits for the
 * events of that thread's LAST scan and returns one entry per launch (at most `capacity`; *n_out = launches).  plane_rows =
 * plane rows the launch streams (each once, row_words * 8 bytes), filters = filter rows it holds in registers. */
typedef struct silo_gpu_scan_timing {
   char kernel[64];       /* e.g. "k_scan_sliced<2, 2, 8, 1, 2>", as rocprofv3 names it; ", pruning" behind k_scan_escapes_sliced<N> where the
                             launch may skip granules of keys and behind k_scan_sliced<2, 2, ..., 2> where it may skip one-hot rows
                             (silo_gpu_mutations_scan_ranges_min_proportion); ", ends" behind either where a range of the launch counts the
                             end runs of the gap symbol (k_scan_sliced leaves the covered rows out, k_scan_escapes_sliced streams the end
                             events and the residual keys); plane_rows and bytes stay those of ALL its rows */
   uint64_t plane_rows;   /* plane rows a k_scan_sliced launch streams (0 for the other kernels) */
   uint64_t bytes;        /* what the launch has to read, each byte once: plane rows + filter rows; 8 bytes per escape key (+ a filter
                             slice per item of k_scan_escapes_sliced, however many blocks walk the items); 12 bytes per run of the missing
                             symbol; 8 per sparse key */
   uint32_t filters;
   uint32_t blocks;       /* of the grid as launched */
   float ms;
} silo_gpu_scan_timing;
int silo_gpu_scan_timings(silo_gpu_scan_timing* out, uint32_t capacity, uint32_t* n_out);

/* The achievable HBM read rate of this device (measurement only; SURVEY.md section 8(d): "also measure an achievable-stream-read
 * ceiling with a plain uint64 sum kernel"): allocates `bytes` of device memory, sums it `reps` times with 16-byte non-temporal
 * loads (8 in flight per lane) and returns the average duration of one pass in *out_ms_per_pass (HIP events, null stream). */
int silo_gpu_stream_read_probe(uint64_t bytes, uint32_t reps, float* out_ms_per_pass);

/* Thread-local description of the last error. */
const char* silo_gpu_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SILO_GPU_H */
