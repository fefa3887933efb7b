// query_engine.h — host-side mirror of silo::query_engine (same type and member names, same error
// behaviour); the arithmetic behind Operator::evaluate and Action::execute runs in HIP kernels.
//
// Reference interfaces mirrored (file:line under the reference tree):
//   QueryEngine::executeQuery            include/silo/query_engine/query_engine.h:13-23, src/.../query_engine.cpp:30-68
//   Query                                src/silo/query_engine/query.cpp:13-28
//   QueryResult / QueryResultEntry       include/silo/query_engine/query_result.h:14-20, src/.../query_result.cpp:10-25
//   OperatorResult                       include/silo/query_engine/operator_result.h:8-31
//   QueryParseException / CHECK_SILO_QUERY   include/silo/query_engine/query_parse_exception.h:6-16
//   QueryCompilationException            include/silo/query_engine/query_compilation_exception.h
//   operators::Operator + subclasses     include/silo/query_engine/operators/*.h
//   filter_expressions::Expression + subclasses   include/silo/query_engine/filter_expressions/*.h
//   actions::Action, Aggregated, Mutations<S>     include/silo/query_engine/actions/{action,aggregated,mutations}.h
#pragma once

#include <cstdint>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <variant>
#include <vector>

#include "database.h"
#include "json.h"

namespace silo {

class QueryParseException : public std::runtime_error {
  public:
   explicit QueryParseException(const std::string& error_message) : std::runtime_error(error_message) {}
};

class QueryCompilationException : public std::runtime_error {
  public:
   explicit QueryCompilationException(const std::string& error_message) : std::runtime_error(error_message) {}
};

#define CHECK_SILO_QUERY(condition, message)    \
   if (!(condition)) {                          \
      throw silo::QueryParseException(message); \
   }

namespace query_engine {

struct QueryResultEntry {
   std::map<std::string, std::optional<std::variant<std::string, int32_t, double>>> fields;
};

struct QueryResult {
   std::vector<QueryResultEntry> query_result;
};

json::Value toJson(const QueryResult& query_result);  // {"queryResult": [...]}
/// The same document as text, without the intermediate tree.
std::string toJsonText(const QueryResult& query_result);

/// The rows an operator ranges over: the reference passes a bare `row_count`; here it also names
/// the device shard that holds those rows.
struct RowSpace {
   uint32_t row_count = 0;
   const DatabasePartition* partition = nullptr;
};

namespace operators {
class Operator;
struct Cost;
}

/// Result of Operator::evaluate.  The reference holds a (borrowed or owned) roaring bitmap; here the
/// evaluation is deferred: cardinality() runs the fused filter kernel in count-only mode, bitset()
/// materialises the row bitset in HBM (both at most once).
class ProgramBuilder;

class OperatorResult {
  public:
   OperatorResult() = default;
   OperatorResult(RowSpace rows, std::unique_ptr<operators::Operator> root);

   [[nodiscard]] uint32_t cardinality() const;
   [[nodiscard]] const uint64_t* bitset() const;  // device pointer, Wp words
   [[nodiscard]] bool isFull() const;              // cardinality() == row_count
   [[nodiscard]] const RowSpace& rows() const;
   /// Runs the kernel now, producing both the bitset and the count in one launch.
   void materialize() const;
   /// Batched counting (QueryEngine::executeQueries): lowers the operator tree into `builder` and hands out the
   /// program, to be launched together with those of other queries (silo_gpu_filter_eval_batch); the caller reports
   /// the cardinality back with setCount.  false: nothing to launch (Empty / Full / already counted).
   [[nodiscard]] bool prepareCount(ProgramBuilder& builder, silo_gpu_bitprog& program) const;
   void setCount(uint32_t count) const;

  private:
   struct State;
   std::shared_ptr<State> state;
};

// ---------------------------------------------------------------------------------------------
// Lowering of an operator tree to the bit-program of include/silo_gpu.h (one fused kernel launch).
// ---------------------------------------------------------------------------------------------
class ProgramBuilder {
  public:
   explicit ProgramBuilder(RowSpace rows) : rows(rows) {}
   ProgramBuilder(const ProgramBuilder&) = delete;
   ProgramBuilder& operator=(const ProgramBuilder&) = delete;
   /// Waits for the stream that temporaryBuffer()s were handed out on, unless run() / runCounting() has: a lowering that throws half
   /// way leaves launches in flight that read and write them.
   ~ProgramBuilder();

   uint32_t allocSlot();
   uint32_t allocRun(uint32_t count);
   void freeSlot(uint32_t slot);
   void freeRun(uint32_t slot, uint32_t count);
   void emit(uint32_t op, uint32_t dst, uint32_t a = 0, uint32_t b = 0, uint32_t imm = 0);
   uint32_t leaf(const uint64_t* device_bitset);
   /// Leaf for a symbol that is stored sparsely: scattered into a cached / pooled bitset before launch.
   uint32_t sparseLeaf(uint32_t seqstore_id, uint32_t position, uint32_t symbol);
   const uint64_t* sparsePointer(uint32_t seqstore_id, uint32_t position, uint32_t symbol);
   /// A row bitset from the partition's pool that lives as long as this builder (filled by the caller before run()).
   uint64_t* temporaryBitset();
   /// `bytes` of device memory from the partition's pool with the same lifetime, for a lowering whose launches on queryStream()
   /// need more than a bitset (DistanceSelection: the table of distances and its scratch).  queuedDeviceWork() holds for it too.
   void* temporaryBuffer(size_t bytes);
   /// Keeps a result whose bitset launches of this lowering read (SampleSelection: the child's rows in the OTHER partitions) as long as
   /// the builder's own buffers: it returns to its pool behind the same wait.
   void keep(OperatorResult result);
   /// Appends `columns` as consecutive leaves; returns the imm of an n-ary instruction (first | count << 16).
   uint32_t leafRun(const std::vector<const uint64_t*>& columns);
   /// Children that are stored columns (foldable by one n-ary instruction) vs composite sub-trees.
   struct Split {
      std::vector<const uint64_t*> columns;
      std::vector<const operators::Operator*> composite;
   };
   Split split(const std::vector<std::unique_ptr<operators::Operator>>& children);
   /// Lowers `child` into this program, or — when it would not fit the instruction / leaf / slot budget that is left —
   /// evaluates it with launches of its own and loads the result as a leaf.
   uint32_t lowerChild(const operators::Operator& child);
   uint32_t lowerChild(const operators::Operator& child, const operators::Cost& cost);  // with child.cost() at hand

   // An expression that needs more than one device program is evaluated in pieces.  Only the node that was lowered into an
   // EMPTY builder (the root of a program, or the only child of such a node) may cut: nothing but its own accumulator is live
   // then.  Every other node was let into the program by lowerChild because its whole cost fitted, so it never needs to.
   /// Nothing lowered so far: the node that begins now may flush().
   [[nodiscard]] bool empty() const { return code.empty() && leaves.empty() && used_slots == 0; }
   /// Whether a sub-tree of this cost fits what is left of the program (with room for the parent to combine it).
   [[nodiscard]] bool fits(const operators::Cost& cost) const;
   /// Room for `leaves` more leaves and `instructions` more instructions (besides the final MOV)?
   [[nodiscard]] bool hasRoom(uint32_t leaves, uint32_t instructions) const;
   /// The leaves that are left.
   [[nodiscard]] size_t leafRoom() const;
   /// Runs the program so far with `operand` as its result into a temporary bitset, starts a fresh program and returns
   /// that bitset as its first leaf operand.  Only for the node that began in an empty() builder.
   uint32_t flush(uint32_t operand);
   /// flush() for `planes` results of one program (the planes of a Threshold's counter, slots first .. first+planes-1): one
   /// launch per plane.  Starts a fresh program; the bitsets are NOT leaves of it yet.
   std::vector<const uint64_t*> flushPlanes(uint32_t first, uint32_t planes);
   /// acc = acc `op` operand, in place where one of the two is a slot (acc == NO_OPERAND: acc = operand).
   static constexpr uint32_t NO_OPERAND = ~0u;
   void combine(uint32_t& acc, uint32_t op, uint32_t operand);
   /// acc = acc `op` fold_n(columns): one n-ary instruction where the run fits the program; in a builder that `may_flush`, runs
   /// of what fits with a flush() between them (both folds are associative, and so is ANDNOT of an OR-run).
   void foldColumns(uint32_t& acc, uint32_t fold_n, uint32_t op, const std::vector<const uint64_t*>& columns, bool may_flush);
   /// lowerChild for a composite child of an n-ary node whose value so far is `acc`: when the child does not fit what is left,
   /// but more would be left after a flush() of the accumulator, it flushes first.  (A child that fits no program is then
   /// evaluated on its own by lowerChild.)
   uint32_t lowerChildBeside(uint32_t& acc, const operators::Operator& child, bool may_flush);

   /// Launches the program (result expected in `result_slot`).
   void run(uint32_t result_slot, uint64_t* out_bitset, uint64_t* out_count, void* stream);
   /// Launches the program and returns the cardinality of its result, delivered by the kernel itself through this
   /// thread's count slot (no counter memset, no device-to-host copy, no stream synchronisation).
   uint32_t runCounting(uint32_t result_slot, uint64_t* out_bitset, void* stream);

   /// Lowering queued device work of its own on the lowering thread's stream (metadata predicates, insertion searches
   /// write temporary bitsets): a program that is launched from ANOTHER stream has to wait for that work first.
   [[nodiscard]] bool queuedDeviceWork() const { return !temporaries.empty(); }
   /// The finished program (result expected in `result_slot`); points into this builder, which must outlive its use.
   silo_gpu_bitprog finishProgram(uint32_t result_slot);

   const RowSpace rows;

  private:
   void restart();  // a fresh program; buffers and materialised children stay with the builder
   std::vector<uint32_t> code;
   std::vector<const uint64_t*> leaves;
   std::vector<DeviceBuffer> temporaries;
   std::vector<OperatorResult> materialized_children;
   void* buffer_stream = nullptr;  // the stream of temporaryBuffer()s nobody has waited for yet
   bool has_buffers = false;
   uint32_t used_slots = 0;  // bit mask
   uint32_t high_water = 0;
};

namespace operators {

enum Type {
   EMPTY, FULL, INDEX_SCAN, INTERSECTION, COMPLEMENT, RANGE_SELECTION, SELECTION, BITMAP_SELECTION, THRESHOLD, UNION, BITMAP_PRODUCER, DISTANCE_SELECTION, SAMPLE_SELECTION, DISTINCT_SELECTION, CELL_COUNT_SELECTION, REGION_CELL_COUNT_SELECTION
};

/// What lowering a sub-tree into a program takes at most.  `slots`: the slots that are live at once while it is lowered, its
/// result included; 0 says that the result is a leaf operand.
struct Cost {
   uint32_t instructions = 0;
   uint32_t leaves = 0;
   uint32_t slots = 0;
};

class Operator {
  public:
   explicit Operator(RowSpace rows) : rows(rows) {}
   virtual ~Operator() noexcept = default;

   [[nodiscard]] virtual Type type() const = 0;
   virtual OperatorResult evaluate() const;
   /// The same for a tree nobody else needs any more: the result takes the tree over instead of copying it.
   static OperatorResult evaluate(std::unique_ptr<Operator> root);
   virtual std::string toString() const = 0;
   virtual std::unique_ptr<Operator> copy() const = 0;
   virtual std::unique_ptr<Operator> negate() const = 0;

   /// Emits this subtree into `builder`; returns the slot (or leaf operand) that holds its value.
   virtual uint32_t lower(ProgramBuilder& builder) const = 0;
   /// Device pointer when this operator is just a stored column (IndexScan, BitmapSelection CONTAINS).
   virtual const uint64_t* storedColumn(ProgramBuilder& /*builder*/) const { return nullptr; }
   [[nodiscard]] virtual Cost cost() const = 0;

   const RowSpace rows;
};

using OperatorVector = std::vector<std::unique_ptr<Operator>>;

class Empty : public Operator {
  public:
   explicit Empty(RowSpace rows) : Operator(rows) {}
   Type type() const override { return EMPTY; }
   std::string toString() const override { return "Empty"; }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 0, 1}; }
};

class Full : public Operator {
  public:
   explicit Full(RowSpace rows) : Operator(rows) {}
   Type type() const override { return FULL; }
   std::string toString() const override { return "Full"; }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 0, 1}; }
};

/// index_scan.cpp: borrows a stored bitmap; here a dense plane pointer in HBM, or a sparse symbol.
class IndexScan : public Operator {
  public:
   IndexScan(const uint64_t* bitmap, RowSpace rows) : Operator(rows), bitmap(bitmap) {}
   IndexScan(uint32_t seqstore_id, uint32_t position, uint32_t symbol, RowSpace rows)
       : Operator(rows), sparse(true), seqstore_id(seqstore_id), position(position), symbol(symbol) {}
   Type type() const override { return INDEX_SCAN; }
   std::string toString() const override { return "IndexScan"; }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   const uint64_t* storedColumn(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   const uint64_t* bitmap = nullptr;
   bool sparse = false;
   uint32_t seqstore_id = 0, position = 0, symbol = 0;
   /// Owner of `bitmap` when it is a plane received from another rank (position-range sharding).
   std::shared_ptr<DeviceBuffer> received;
};

/// bitmap_selection.cpp probes the row-wise missing-symbol bitmaps; the dense store keeps the missing
/// symbol as a column plane, so CONTAINS is that plane and NOT_CONTAINS its complement.
class BitmapSelection : public Operator {
  public:
   enum Comparator { CONTAINS, NOT_CONTAINS };
   BitmapSelection(const uint64_t* missing_plane, RowSpace rows, Comparator comparator, uint32_t value)
       : Operator(rows), missing_plane(missing_plane), comparator(comparator), value(value) {}
   /// The missing symbol of a store that keeps it as runs (no resident plane): the position's plane is materialised, and
   /// cached, when the operator is lowered — like a sparsely stored symbol of an IndexScan.
   BitmapSelection(uint32_t seqstore_id, uint32_t local_position, uint32_t symbol, RowSpace rows, Comparator comparator, uint32_t value)
       : Operator(rows), missing_plane(nullptr), comparator(comparator), value(value), materialise(true), seqstore_id(seqstore_id),
         local_position(local_position), symbol(symbol) {}
   Type type() const override { return BITMAP_SELECTION; }
   std::string toString() const override { return "BitmapSelection"; }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   const uint64_t* storedColumn(ProgramBuilder& builder) const override;
   Cost cost() const override { return {2, 1, comparator == CONTAINS ? 0u : 1u}; }

   const uint64_t* missing_plane;
   Comparator comparator;
   uint32_t value;  // the position, kept for parity with the reference's constructor
   bool materialise = false;
   uint32_t seqstore_id = 0;
   uint32_t local_position = 0;
   uint32_t symbol = 0;
};

class Complement : public Operator {
  public:
   Complement(std::unique_ptr<Operator> child, RowSpace rows) : Operator(rows), child(std::move(child)) {}
   Type type() const override { return COMPLEMENT; }
   std::string toString() const override { return "!" + child->toString(); }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override;

   std::unique_ptr<Operator> child;
};

class Intersection : public Operator {
  public:
   Intersection(OperatorVector&& children, OperatorVector&& negated_children, RowSpace rows);
   Type type() const override { return INTERSECTION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override;

   OperatorVector children;
   OperatorVector negated_children;
};

class Union : public Operator {
  public:
   Union(OperatorVector&& children, RowSpace rows) : Operator(rows), children(std::move(children)) {}
   Type type() const override { return UNION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override;

   OperatorVector children;
};

/// One comparison of a metadata column with a constant (CompareToValueSelection<T>, selection.h:52-70): on the
/// device a k_bitset_from_compare launch that turns the column into a row bitset.
struct Predicate {
   const storage::column::MetadataColumnPartition* column;
   int comparator;  // SILO_GPU_CMP_*
   union {
      int32_t as_int;
      uint32_t as_word;
      double as_double;
   } value;
   [[nodiscard]] Predicate negated() const;  // the comparator is negated, selection.cpp:195-220
};

/// selection.cpp: rows (of `child`, or all) that satisfy every predicate.
class Selection : public Operator {
  public:
   Selection(std::unique_ptr<Operator> child, std::vector<Predicate> predicates, RowSpace rows)
       : Operator(rows), child(std::move(child)), predicates(std::move(predicates)) {}
   Selection(std::vector<Predicate> predicates, RowSpace rows) : Operator(rows), predicates(std::move(predicates)) {}
   Type type() const override { return SELECTION; }
   std::string toString() const override { return "Select[" + std::to_string(predicates.size()) + " predicates]"; }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override;

   std::unique_ptr<Operator> child;  // may be null
   std::vector<Predicate> predicates;
};

/// bitmap_producer.cpp: a bitmap computed at evaluation time.  The only producer on this path is the insertion
/// search (insertion_contains.cpp:104-113): the rows that carry one of the distinct insertions the pattern matched,
/// scattered into a bitset by k_bitset_from_pairs.
class BitmapProducer : public Operator {
  public:
   BitmapProducer(const storage::column::InsertionColumnPartition::SequenceIndex* index, std::vector<uint8_t> membership, RowSpace rows)
       : Operator(rows), index(index), membership(std::move(membership)) {}
   Type type() const override { return BITMAP_PRODUCER; }
   std::string toString() const override { return "BitmapProducer"; }
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   const storage::column::InsertionColumnPartition::SequenceIndex* index;
   std::vector<uint8_t> membership;  // per distinct insertion id of the index
};

/// The rows within a distance of one query sequence (the filter expression WithinDistance; no counterpart in the reference): a
/// bitmap computed at evaluation time like BitmapProducer's.  lower() leaves (distance, compared) of every row of the partition in
/// a pooled table (silo_gpu_query_distances, K11) and turns it into a row bitset on the device (silo_gpu_bitset_from_distances),
/// both on the lowering thread's stream ahead of the fused program, which reads the bitset as a leaf.  The table, its scratch and
/// the bitset belong to the builder: nothing returns to the pool before the stream has been waited for.
class DistanceSelection : public Operator {
  public:
   DistanceSelection(uint32_t seqstore_id, std::string query, uint32_t max_distance, uint32_t min_compared, RowSpace rows)
       : Operator(rows), seqstore_id(seqstore_id), query(std::move(query)), max_distance(max_distance), min_compared(min_compared) {}
   Type type() const override { return DISTANCE_SELECTION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   uint32_t seqstore_id;
   std::string query;  // the aligned query sequence, one character per position of the sequence store
   uint32_t max_distance;
   uint32_t min_compared;
};

/// A seeded random subset of the rows a child selects (the filter expression Sample; no counterpart in the reference): the `size`
/// rows with the smallest keys of a keyed permutation of the database's row numbers — of the whole selection, or of each date range.
/// The selection is one over ALL partitions, so the operator of a partition holds the child of every partition: lower() evaluates
/// each of them, finds every group's threshold with K19 (silo_gpu_sample_begin, four rounds of silo_gpu_sample_count per partition
/// and silo_gpu_sample_advance) without a host round trip, and writes its own partition's bitset (silo_gpu_sample_select), all on
/// the lowering thread's stream ahead of the fused program, which reads the bitset as a leaf.  The state, the group arrays and the
/// children's results belong to the builder, like DistanceSelection's buffers: nothing returns to a pool before the stream has
/// been waited for.
class SampleSelection : public Operator {
  public:
   /// A partition of the database that has rows, in the database's order.
   struct Part {
      std::unique_ptr<Operator> child;
      const uint32_t* dates = nullptr;  // the date column's values on the device; null without date ranges
      uint32_t first_row = 0;           // the number of the partition's first row in the database
   };
   SampleSelection(std::vector<Part> parts, uint32_t own, uint32_t size, uint64_t seed, std::vector<uint32_t> range_bounds, RowSpace rows)
       : Operator(rows), parts(std::move(parts)), own(own), size(size), seed(seed), range_bounds(std::move(range_bounds)) {}
   Type type() const override { return SAMPLE_SELECTION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   std::vector<Part> parts;
   uint32_t own;  // the part this operator answers for
   uint32_t size;
   uint64_t seed;
   std::vector<uint32_t> range_bounds;  // (from, to) per date range as K7 takes them; empty: one group of all rows
};

/// One row per distinct aligned sequence among the rows a child selects (the filter expression DistinctSequences; no counterpart in
/// the reference): of every class of rows with equal 128-bit row hashes (K20) the row with the smallest number in the database.  Like
/// SampleSelection the choice is one over ALL partitions, so the operator of a partition holds the child of every partition:
/// lower() evaluates each of them, takes every store's kept hashes (silo_gpu_store_row_hashes: the first query on a store computes
/// them), fills one owner table (silo_gpu_distinct_begin, silo_gpu_distinct_insert per partition) and writes its own partition's
/// bitset (silo_gpu_distinct_select), all on the lowering thread's stream ahead of the fused program, which reads the bitset as a
/// leaf.  The table, the uploaded parts and the children's results belong to the builder, like SampleSelection's.
class DistinctSelection : public Operator {
  public:
   /// A partition of the database that has rows, in the database's order.
   struct Part {
      std::unique_ptr<Operator> child;
      uint32_t seqstore_id = 0;  // of the compared sequence in this partition's store
      uint32_t first_row = 0;    // the number of the partition's first row in the database
   };
   DistinctSelection(std::vector<Part> parts, uint32_t own, uint64_t database_rows, RowSpace rows)
       : Operator(rows), parts(std::move(parts)), own(own), database_rows(database_rows) {}
   Type type() const override { return DISTINCT_SELECTION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   std::vector<Part> parts;
   uint32_t own;            // the part this operator answers for
   uint64_t database_rows;  // what the owner table is sized for
};

/// K20's owner table over the rows that a filter selects in every partition that has rows — what DistinctSelection::lower and the
/// action DistinctSequenceCounts (distance_actions.cpp) both begin with.  buildDistinctTable takes each partition in the database's
/// order: its rows (`rows_of(part)`: the caller evaluates or hands over the filter's bitset and keeps it alive), then its store's
/// kept row hashes (silo_gpu_store_row_hashes: the first query on a store computes them and waits).  It sizes the table as the
/// smallest power of two >= 2 x database_rows slots, uploads the parts and enqueues silo_gpu_distinct_begin and one
/// silo_gpu_distinct_insert per partition on queryStream().  The two device arrays come from `allocate` and belong to the caller:
/// they must outlive the wait for the stream.  `what` names the caller in the refusal of a table of more than 2^31 slots.
struct DistinctTable {
   /// A partition of the database that has rows, in the database's order.
   struct Part {
      const DatabasePartition* partition;
      uint32_t seqstore_id;  // of the compared sequence in this partition's store
      uint32_t first_row;    // the number of the partition's first row in the database
   };
   silo_gpu_distinct_part* device_parts = nullptr;
   void* table = nullptr;  // SILO_GPU_DISTINCT_TABLE_BYTES(slots)
   uint32_t slots = 0;
   uint32_t n_parts = 0;
   std::vector<const uint64_t*> filters;  // per part, as rows_of returned them
};
DistinctTable buildDistinctTable(
   const std::vector<DistinctTable::Part>& parts, uint64_t database_rows, const std::function<const uint64_t*(size_t part)>& rows_of,
   const std::function<void*(size_t bytes)>& allocate, const std::string& what
);

/// The rows whose cell counts against the reference — substitutions, deletions, missing, ambiguous (K22) — sum, over the kinds of
/// `kinds_mask`, to a value in [at_least, at_most] (the filter expression CellCount; no counterpart in the reference).  lower() takes
/// the store's kept table of cell counts (silo_gpu_store_row_cell_counts: the first query on a store computes it and waits, so that
/// request pays for the build) and turns it into a row bitset on the device (silo_gpu_bitset_from_cell_counts) on the lowering
/// thread's stream ahead of the fused program, which reads the bitset as a leaf.  The bitset belongs to the builder, like
/// DistanceSelection's buffers; the table belongs to the store.
class CellCountSelection : public Operator {
  public:
   CellCountSelection(uint32_t seqstore_id, uint32_t kinds_mask, uint32_t at_least, uint32_t at_most, RowSpace rows)
       : Operator(rows), seqstore_id(seqstore_id), kinds_mask(kinds_mask), at_least(at_least), at_most(at_most) {}
   Type type() const override { return CELL_COUNT_SELECTION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   uint32_t seqstore_id;
   uint32_t kinds_mask;  // SILO_GPU_CELL_COUNT_* bits
   uint32_t at_least;
   uint32_t at_most;
};

/// The rows whose number of cells of the kinds of `kinds_mask` at the positions [first, end) (0-based) lies in [at_least, at_most]:
/// the filter expression CellCount with positionFrom / positionTo (K23; no counterpart in the reference).  lower() computes the
/// region's column of values (silo_gpu_region_cell_values, one range) and turns it into a row bitset (silo_gpu_bitset_from_values)
/// on the lowering thread's stream ahead of the fused program, which reads the bitset as a leaf.  The column, the scratch and the
/// bitset belong to the builder, like DistanceSelection's buffers; the store keeps nothing.
class RegionCellCountSelection : public Operator {
  public:
   RegionCellCountSelection(uint32_t seqstore_id, uint32_t positions, uint32_t first, uint32_t end, uint32_t kinds_mask, uint32_t at_least, uint32_t at_most, RowSpace rows)
       : Operator(rows), seqstore_id(seqstore_id), positions(positions), first(first), end(end), kinds_mask(kinds_mask), at_least(at_least), at_most(at_most) {}
   Type type() const override { return REGION_CELL_COUNT_SELECTION; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override { return {1, 1}; }

   uint32_t seqstore_id;
   uint32_t positions;   // of the sequence: sizes the scratch
   uint32_t first, end;  // 0-based, half-open
   uint32_t kinds_mask;  // SILO_GPU_CELL_COUNT_* bits
   uint32_t at_least;
   uint32_t at_most;
};

class Threshold : public Operator {
  public:
   Threshold(OperatorVector&& non_negated_children, OperatorVector&& negated_children, uint32_t number_of_matchers, bool match_exactly, RowSpace rows);
   Type type() const override { return THRESHOLD; }
   std::string toString() const override;
   std::unique_ptr<Operator> copy() const override;
   std::unique_ptr<Operator> negate() const override;
   uint32_t lower(ProgramBuilder& builder) const override;
   Cost cost() const override;

   OperatorVector non_negated_children;
   OperatorVector negated_children;
   uint32_t number_of_matchers;
   bool match_exactly;

  private:
   /// lower() for the root of a program whose children may not fit it: as many programs as they need.
   uint32_t lowerInPieces(ProgramBuilder& builder, const ProgramBuilder::Split& positive, const ProgramBuilder::Split& negative, uint32_t bits) const;
};

}  // namespace operators

namespace filter_expressions {

struct Expression {
   enum AmbiguityMode { UPPER_BOUND, LOWER_BOUND, NONE };
   virtual ~Expression() = default;
   virtual std::string toString(const Database& database) const = 0;
   [[nodiscard]] virtual std::unique_ptr<operators::Operator> compile(
      const Database& database, const DatabasePartition& database_partition, AmbiguityMode mode
   ) const = 0;
};

Expression::AmbiguityMode invertMode(Expression::AmbiguityMode mode);

/// expression.cpp:49-102
std::unique_ptr<Expression> parseExpression(const json::Value& json);

using ExpressionVector = std::vector<std::unique_ptr<Expression>>;

#define SILO_DECLARE_EXPRESSION_METHODS                                        \
   std::string toString(const Database& database) const override;            \
   [[nodiscard]] std::unique_ptr<operators::Operator> compile(                 \
      const Database& database, const DatabasePartition& database_partition, AmbiguityMode mode \
   ) const override;

struct True : public Expression {
   SILO_DECLARE_EXPRESSION_METHODS
};
struct False : public Expression {
   SILO_DECLARE_EXPRESSION_METHODS
};
struct And : public Expression {
   explicit And(ExpressionVector&& children) : children(std::move(children)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   ExpressionVector children;
};
struct Or : public Expression {
   explicit Or(ExpressionVector&& children) : children(std::move(children)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   ExpressionVector children;
};
struct Negation : public Expression {
   explicit Negation(std::unique_ptr<Expression> child) : child(std::move(child)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::unique_ptr<Expression> child;
};
struct Maybe : public Expression {
   explicit Maybe(std::unique_ptr<Expression> child) : child(std::move(child)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::unique_ptr<Expression> child;
};
struct Exact : public Expression {
   explicit Exact(std::unique_ptr<Expression> child) : child(std::move(child)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::unique_ptr<Expression> child;
};
struct NOf : public Expression {
   NOf(ExpressionVector&& children, int number_of_matchers, bool match_exactly)
       : children(std::move(children)), number_of_matchers(number_of_matchers), match_exactly(match_exactly) {}
   SILO_DECLARE_EXPRESSION_METHODS
   ExpressionVector children;
   int number_of_matchers;
   bool match_exactly;
};
struct NucleotideSymbolEquals : public Expression {
   NucleotideSymbolEquals(std::optional<std::string> nuc_sequence_name, uint32_t position, std::optional<Nucleotide::Symbol> value)
       : nuc_sequence_name(std::move(nuc_sequence_name)), position(position), value(value) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::optional<std::string> nuc_sequence_name;
   uint32_t position;
   std::optional<Nucleotide::Symbol> value;
};
struct AASymbolEquals : public Expression {
   AASymbolEquals(std::string aa_sequence_name, uint32_t position, std::optional<AminoAcid::Symbol> value)
       : aa_sequence_name(std::move(aa_sequence_name)), position(position), value(value) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string aa_sequence_name;
   uint32_t position;
   std::optional<AminoAcid::Symbol> value;
};
struct HasMutation : public Expression {
   HasMutation(std::optional<std::string> nuc_sequence_name, uint32_t position)
       : nuc_sequence_name(std::move(nuc_sequence_name)), position(position) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::optional<std::string> nuc_sequence_name;
   uint32_t position;
};
struct HasAAMutation : public Expression {
   HasAAMutation(std::string aa_sequence_name, uint32_t position)
       : aa_sequence_name(std::move(aa_sequence_name)), position(position) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string aa_sequence_name;
   uint32_t position;
};
struct PangoLineageFilter : public Expression {
   PangoLineageFilter(std::string column, std::string lineage, bool include_sublineages)
       : column(std::move(column)), lineage(std::move(lineage)), include_sublineages(include_sublineages) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   std::string lineage;
   bool include_sublineages;
};
// ---- metadata predicates ----
struct StringEquals : public Expression {  // string_equals.cpp
   StringEquals(std::string column, std::string value) : column(std::move(column)), value(std::move(value)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   std::string value;
};
struct IntEquals : public Expression {  // int_equals.cpp
   IntEquals(std::string column, int32_t value) : column(std::move(column)), value(value) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   int32_t value;
};
struct IntBetween : public Expression {  // int_between.cpp
   IntBetween(std::string column, std::optional<int32_t> from, std::optional<int32_t> to) : column(std::move(column)), from(from), to(to) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   std::optional<int32_t> from;
   std::optional<int32_t> to;
};
struct FloatEquals : public Expression {  // float_equals.cpp
   FloatEquals(std::string column, double value) : column(std::move(column)), value(value) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   double value;
};
struct FloatBetween : public Expression {  // float_between.cpp
   FloatBetween(std::string column, std::optional<double> from, std::optional<double> to) : column(std::move(column)), from(from), to(to) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   std::optional<double> from;
   std::optional<double> to;
};
template <typename SymbolType>
struct InsertionContains : public Expression {  // insertion_contains.cpp
   InsertionContains(std::vector<std::string>&& column_names, std::optional<std::string> sequence_name, uint32_t position, std::string value)
       : column_names(std::move(column_names)), sequence_name(std::move(sequence_name)), position(position), value(std::move(value)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::vector<std::string> column_names;
   std::optional<std::string> sequence_name;
   uint32_t position;
   std::string value;
};
/// WithinDistance (no counterpart in the reference): the rows at most maxDistance away from one query sequence — a row named by its
/// primary key (which the selection contains: it is at distance 0 from itself) or a literal aligned string — with at least
/// minComparedPositions positions compared, by the distance of DistanceMatrix / NearestNeighbours on one aligned sequence.  The
/// parsed expression holds only what the query text says: compile resolves the query's characters against the database it is given.
struct WithinDistance : public Expression {
   WithinDistance(
      std::optional<std::string> sequence_name, std::optional<json::Value> primary_key, std::optional<std::string> sequence, uint32_t max_distance,
      uint32_t min_compared_positions
   )
       : sequence_name(std::move(sequence_name)),
         primary_key(std::move(primary_key)),
         sequence(std::move(sequence)),
         max_distance(max_distance),
         min_compared_positions(min_compared_positions) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::optional<json::Value> primary_key;    // exactly one of the two
   std::optional<std::string> sequence;
   uint32_t max_distance;
   uint32_t min_compared_positions;
};
/// Sample (no counterpart in the reference): `size` rows of the child's selection over the WHOLE database, chosen by the order of
/// key(seed, global row number) — or, with dateField and dateRanges, at most `size` rows of each date range (both ends inclusive, a
/// NULL date in no range; rows of the child in no range are not selected).  The selection depends on the seed, the child's rows and
/// their numbers in the database alone, not on how the rows are cut into partitions.  The child is compiled in the mode Sample is
/// compiled in, for every partition: P partitions compile and evaluate it P times each (no state is kept between them).
struct Sample : public Expression {
   Sample(std::unique_ptr<Expression> child, uint32_t size, uint64_t seed, std::optional<std::string> date_field, std::vector<uint32_t> range_bounds)
       : child(std::move(child)), size(size), seed(seed), date_field(std::move(date_field)), range_bounds(std::move(range_bounds)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::unique_ptr<Expression> child;
   uint32_t size;
   uint64_t seed;
   std::optional<std::string> date_field;  // with it: range_bounds, (from, to) per range as K7 takes them
   std::vector<uint32_t> range_bounds;
};
/// DistinctSequences (no counterpart in the reference): of the rows the child selects over the WHOLE database, one per distinct
/// aligned sequence of `sequence_name` (the default nucleotide sequence when absent) — the row with the smallest number in the
/// database of every class of rows with equal row hashes (K20: 128 bits; rows with equal hashes are treated as identical).  The
/// selection depends on the child's rows, their sequences and their numbers in the database alone.  The child is compiled in the mode
/// DistinctSequences is compiled in, for every partition, as for Sample.
struct DistinctSequences : public Expression {
   DistinctSequences(std::unique_ptr<Expression> child, std::optional<std::string> sequence_name)
       : child(std::move(child)), sequence_name(std::move(sequence_name)) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::unique_ptr<Expression> child;
   std::optional<std::string> sequence_name;
};
/// CellCount (no counterpart in the reference): the rows whose number of cells of the listed kinds — substitutions, deletions,
/// missing, ambiguous against the reference of `sequence_name` (the default nucleotide sequence when absent), the four counts of
/// MutationsPerSequence over all positions — lies in [at_least, at_most].  An absent bound is 0 / 2^32 - 1.  The parsed expression
/// holds only what the query text says; compile answers what the number of positions alone decides without touching the store.
/// With `position_from` / `position_to` (1-based, inclusive; an absent one is 1 / the sequence's length) the cells counted are those
/// of that range of positions alone (K23); a range that is the whole sequence compiles as if neither were given.
struct CellCount : public Expression {
   CellCount(
      std::optional<std::string> sequence_name, uint32_t kinds_mask, uint32_t at_least, uint32_t at_most,
      std::optional<uint32_t> position_from = std::nullopt, std::optional<uint32_t> position_to = std::nullopt
   )
       : sequence_name(std::move(sequence_name)), kinds_mask(kinds_mask), at_least(at_least), at_most(at_most), position_from(position_from),
         position_to(position_to) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   uint32_t kinds_mask;                       // SILO_GPU_CELL_COUNT_* bits
   uint32_t at_least;
   uint32_t at_most;
   std::optional<uint32_t> position_from;     // 1-based
   std::optional<uint32_t> position_to;       // 1-based, inclusive
};
/// The field `cells` of CellCount and CellCountDistribution: one kind or a non-empty list of kinds without repeats, as a mask of
/// SILO_GPU_CELL_COUNT_* bits; anything else is a bad request with the message `complaint` (filter_expressions.cpp).
uint32_t parseCellKinds(const json::Value& cells, const std::string& complaint);
/// "substitutions+missing": the kinds of a mask in their order.
std::string cellKindsString(uint32_t kinds_mask);
struct DateBetween : public Expression {  // date_between.cpp
   DateBetween(std::string column, std::optional<common::Date> date_from, std::optional<common::Date> date_to)
       : column(std::move(column)), date_from(date_from), date_to(date_to) {}
   SILO_DECLARE_EXPRESSION_METHODS
   std::string column;
   std::optional<common::Date> date_from;
   std::optional<common::Date> date_to;
};

}  // namespace filter_expressions

namespace actions {

struct OrderByField {
   std::string name;
   bool ascending;
};

/// Scans of several queries that read the same planes are collected here and issued as batched launches
/// (silo_gpu_mutations_scan_batch: one pass over the planes for up to 4 filters).  A batcher is active on a
/// thread only inside QueryEngine::executeQueries; otherwise every scan is launched at once.
class ScanBatcher {
  public:
   struct Request {
      silo_gpu_store* store;
      uint32_t seqstore_id;
      const uint64_t* filter;  // nullptr = full filter
      uint32_t pos_begin, pos_end;
      uint32_t* counts;
      /// > 0: the table is read by the row selection of a Mutations action with this minProportion and by nothing else, and no
      /// other scan adds into this store's part of it — the scan may then leave out escape keys that cannot reach the proportion
      /// (silo_gpu_mutations_scan_ranges_min_proportion).  0: every cell exact.
      double min_proportion = 0;
      /// slot != nullptr: this scan is the ONLY writer of the query's count table (sink.table_dev, which `counts` points into) and
      /// the row selection with min_proportion its only reader — the scans of the query leave in a call that overwrites the table
      /// and delivers the selected rows into the slot (silo_gpu_mutations_scan_select); the table is not cleared beforehand.
      silo_gpu_select_sink sink{};
   };
   ScanBatcher();
   ~ScanBatcher();
   ScanBatcher(const ScanBatcher&) = delete;
   static ScanBatcher* active();
   void add(const Request& request) { requests.push_back(request); }
   /// With collectives installed: sum `n` counts across ranks after the scans of the batch were launched
   /// (every rank runs the same batch, so the reductions pair up in recording order).
   void addReduction(const Database& database, uint32_t* device_values, size_t n) { reductions.push_back({&database, device_values, n}); }
   /// Work that has to follow the launches (and reductions) of the batch on the stream, e.g. fetching the results.
   void afterFlush(std::function<void()> callback) { after_flush.push_back(std::move(callback)); }
   /// What a query recorded can be dropped again when it fails before the flush (its buffers die with it).
   struct Checkpoint {
      size_t requests, reductions, after_flush;
   };
   [[nodiscard]] Checkpoint checkpoint() const { return {requests.size(), reductions.size(), after_flush.size()}; }
   void rollback(const Checkpoint& mark) {
      requests.resize(mark.requests);
      reductions.resize(mark.reductions);
      after_flush.resize(mark.after_flush);
   }
   void flush();

  private:
   struct Reduction {
      const Database* database;
      uint32_t* device_values;
      size_t n;
   };
   std::vector<Request> requests;
   std::vector<Reduction> reductions;
   std::vector<std::function<void()>> after_flush;
   ScanBatcher* previous;
};

class Action {
  protected:
   std::vector<OrderByField> order_by_fields;
   std::optional<uint32_t> limit;
   std::optional<uint32_t> offset;

   void applySort(QueryResult& result) const;
   void applyOffsetAndLimit(QueryResult& result) const;
   virtual void validateOrderByFields(const Database& database) const = 0;
   /// For validateOrderByFields of an action whose rows have a fixed set of fields: every field ordered by is one of `fields`.
   void checkOrderByFields(std::initializer_list<std::string_view> fields) const;
   [[nodiscard]] virtual QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const = 0;

  public:
   /// State of an action between its two phases (see begin / finish).
   struct Pending {
      virtual ~Pending() = default;
      std::vector<OperatorResult> bitmap_filter;
   };

   virtual ~Action() = default;
   /// The action needs nothing but the cardinality of the filter (Aggregated without groupByFields): a batch of such
   /// queries evaluates all its filters in one launch.
   [[nodiscard]] virtual bool countsOnly() const { return false; }
   void setOrdering(const std::vector<OrderByField>& order_by_fields, std::optional<uint32_t> limit, std::optional<uint32_t> offset);
   [[nodiscard]] virtual QueryResult executeAndOrder(const Database& database, std::vector<OperatorResult> bitmap_filter) const;

   /// Two-phase form of executeAndOrder for batches of queries: begin() validates and queues the device
   /// work (with a ScanBatcher active the scans are only recorded), finish() fetches the results, builds the
   /// rows and applies ordering / offset / limit.  The default runs everything in finish().
   [[nodiscard]] virtual std::unique_ptr<Pending> begin(const Database& database, std::vector<OperatorResult> bitmap_filter) const;
   [[nodiscard]] virtual QueryResult finish(const Database& database, Pending& pending) const;
   /// finish() as the response body — the bytes of toJsonText(finish(...)).  An action whose rows come off the device as
   /// plain numbers (Mutations) writes them straight into the text: the map-of-variants rows the reference's QueryResult
   /// prescribes (query_result.h:14-20) cost more to build than the whole scan of a small query takes.
   [[nodiscard]] virtual std::string finishJson(const Database& database, Pending& pending) const;

  protected:
   [[nodiscard]] QueryResult orderAndLimit(QueryResult result) const;
};

/// action.cpp:144-187
std::unique_ptr<Action> parseAction(const json::Value& json);
/// The parsers of the count-table actions (table_actions.cpp), which parseAction's table of action types names.
template <typename SymbolType>
std::unique_ptr<Action> parseMutationsOverTime(const json::Value& json);
std::unique_ptr<Action> parseQueriesOverTime(const json::Value& json);
std::unique_ptr<Action> parseCrossTabulation(const json::Value& json);
template <typename SymbolType>
std::unique_ptr<Action> parseConsensus(const json::Value& json);
template <typename SymbolType>
std::unique_ptr<Action> parseMutationsComparison(const json::Value& json);
/// The parser of the sums of pairwise distances within and between groups (actions.cpp; execute in table_actions.cpp).
template <typename SymbolType>
std::unique_ptr<Action> parseMeanDistances(const json::Value& json);
/// An entry of a groups field (Consensus, MutationsComparison, MeanDistances) as the messages show it, and the entries of such a
/// field (`list`, an array) in request order: objects with a string name that no entry before had and a filterExpression, whose own
/// complaint comes behind the field and the group (table_actions.cpp).
extern const std::string GROUP_ENTRY_FORM;
std::vector<std::pair<std::string, std::unique_ptr<filter_expressions::Expression>>> parseGroupEntries(const json::Value& list, const std::string& action_name);
/// The parsers of the sequence-comparing actions (distance_actions.cpp).
std::unique_ptr<Action> parseDistanceMatrix(const json::Value& json);
std::unique_ptr<Action> parseClusters(const json::Value& json);
std::unique_ptr<Action> parseMinimumSpanningTree(const json::Value& json);
std::unique_ptr<Action> parseNearestAmong(const json::Value& json);
std::unique_ptr<Action> parseNearestNeighbours(const json::Value& json);
/// The parser of the action over the classes of equal sequences (distance_actions.cpp).
std::unique_ptr<Action> parseDistinctSequenceCounts(const json::Value& json);
/// The parser of the histogram of the selection's cell counts (sequence_actions.cpp).
std::unique_ptr<Action> parseCellCountDistribution(const json::Value& json);
/// The parser of the per-region counts of the selection (sequence_actions.cpp).
std::unique_ptr<Action> parseCellCountByRegion(const json::Value& json);

/// Two kinds of field that many action parsers read, with one wording of the complaint (actions.cpp).  An optional field of type
/// string: none when absent; "<action_name> action: the field <field>, if present, must be of type string".
std::optional<std::string> optionalStringField(const json::Value& json, std::string_view field, const std::string& action_name);
/// An unsigned integer field whose value, read as int64, lies in [minimum, maximum]: none when absent and not `required`.
/// "<action_name> action: the field <field>[, if present,] must be <form>"; a required field that is absent: "... is required".
std::optional<uint32_t> integerField(
   const json::Value& json, std::string_view field, const std::string& action_name, bool required, int64_t minimum, int64_t maximum, const std::string& form
);

/// Refuses a sharded database on behalf of an action whose counts are not all-reduced across ranks (table_actions.cpp).
void requireUnsharded(const Database& database, const std::string& action_name);
/// The metadata column `name` of a partition; a runtime_error if it was not loaded (metadata_actions.cpp).
const storage::column::MetadataColumnPartition& columnOf(const DatabasePartition& partition, const std::string& name);
/// The set bits of a filter, fetched from the device (sequence_actions.cpp).
std::vector<uint32_t> selectedRows(const DatabasePartition& partition, const OperatorResult& filter);
/// The rows the filters select, over all partitions that hold rows (sequence_actions.cpp).
size_t selectedCount(const Database& database, const std::vector<OperatorResult>& bitmap_filter);

/// A sequence store of one alphabet by name, as the templated actions take it: none is the default nucleotide sequence.
template <typename SymbolType>
struct NamedSequenceStore {
   std::string name;
   const SequenceStore<SymbolType>& store;
};
/// `complaint`: the caller's wording of the refusal up to the name, which follows it in single quotes.
template <typename SymbolType>
NamedSequenceStore<SymbolType> sequenceStoreOf(const Database& database, const std::optional<std::string>& sequence_name, const std::string& complaint) {
   std::string name = sequence_name.value_or(database.database_config.default_nucleotide_sequence);
   const auto found = database.getSequenceStores<SymbolType>().find(name);
   CHECK_SILO_QUERY(found != database.getSequenceStores<SymbolType>().end(), complaint + "'" + name + "'")
   return {std::move(name), found->second};
}

/// An aligned sequence of either alphabet by name, as the actions and filters that read characters take it: a nucleotide sequence
/// if there is one of that name, otherwise a gene; none is the default nucleotide sequence (sequence_actions.cpp).
struct AlignedSequence {
   std::string name;
   bool is_amino_acid;
   int alphabet;  // SILO_GPU_ALPHABET_*
   uint32_t positions;
   [[nodiscard]] uint32_t seqstoreOf(const DatabasePartition& partition) const;
};
/// `complaint` as for sequenceStoreOf.
AlignedSequence alignedSequence(const Database& database, const std::optional<std::string>& sequence_name, const std::string& complaint);

/// The walk that every action over the selected rows' sequences begins with (FastaAligned, MutationsPerSequence, and through
/// PackedSelection the distance actions): the rows the filters select, numbered in partition order, then by ascending row id.
/// gather() takes every partition that holds rows and selected rows in turn: it collects the primary keys (a null key as it is),
/// uploads the row ids into a buffer of that partition's pool and hands them to `step`, which enqueues the gather
/// (silo_gpu_reconstruct_sequences) on queryStream().  The object owns the row-id buffers, which those launches read: it is declared
/// BEFORE the waitIfThrown / launchAndWait that gather() is called under, so that it outlives the wait for the stream.
class SelectedSequences {
  public:
   using PartitionRow = std::pair<uint32_t, uint32_t>;
   /// (the partition, its selected row ids on the device, how many, the number of the first of them)
   using Step = std::function<void(const DatabasePartition& partition, const uint32_t* device_rows, uint32_t n_rows, size_t first_sequence)>;
   std::vector<JsonValue> keys;          // the primary keys of sequence 0 .. n - 1
   std::vector<PartitionRow> numbering;  // if `numbered`: their (partition, row id), ascending

   /// n: selectedCount of the filters; a filter that selects more or fewer rows is a runtime_error ("<what>: a filter selects ...").
   /// No `step`: only the keys are collected, nothing is uploaded or launched.
   void gather(const Database& database, const std::vector<OperatorResult>& bitmap_filter, size_t n, const std::string& what, bool numbered, const Step& step);

  private:
   std::vector<DeviceBuffer> row_ids;  // per partition with selected rows
};

/// The rule that keeps a pooled device buffer from being handed to another query while a kernel of this one still uses it, for
/// work enqueued on queryStream() that reads and writes DeviceBuffers declared BEFORE the call (so that they die after it).
/// waitIfThrown runs `launches`; if they throw, launches of this query may be in flight on the stream: it lets them finish before
/// the exception unwinds the buffers back into the pool.  On its own it serves work whose buffers outlive it anyway, or that ends
/// in a synchronous copy.  launchAndWait also waits for the stream when `launches` return — a fetch was the last thing enqueued
/// and has been waited for, but it says so: nothing of this query runs any more when its buffers go back (table_actions.cpp).
void waitIfThrown(const std::function<void()>& launches);
void launchAndWait(const std::function<void()>& launches);

/// The aligned sequence that NearestNeighbours and WithinDistance compare every row with (distance_actions.cpp).
struct QuerySequence {
   std::string characters;             // one per position of the sequence
   size_t own_partition = SIZE_MAX;    // where the row named by a primary key lives; a literal sequence has none
   uint32_t own_row = UINT32_MAX;
};
/// The literal `sequence` (which must have the length of `compared`), or the row whose primary key is `primary_key`:
/// looked up in the host copies of the key column of every partition and gathered from its store (silo_gpu_reconstruct_sequences,
/// n = 1) on the calling thread's queryStream(), which is waited for.  `what` opens every message ("NearestNeighbours action").
QuerySequence resolveQuerySequence(
   const Database& database, const AlignedSequence& compared, const std::optional<json::Value>& primary_key, const std::optional<std::string>& sequence,
   const std::string& what
);

class Aggregated : public Action {
   std::vector<std::string> group_by_fields;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
   /// aggregated.cpp:100-149 — per partition one k_group_count launch over the dictionary ids of the fields
   [[nodiscard]] QueryResult aggregateWithGrouping(const Database& database, std::vector<OperatorResult>& bitmap_filter) const;

  public:
   explicit Aggregated(std::vector<std::string> group_by_fields) : group_by_fields(std::move(group_by_fields)) {}
   [[nodiscard]] bool countsOnly() const override { return group_by_fields.empty(); }
};

/// Haplotypes / AminoAcidHaplotypes: which combinations of symbols occur together at up to MAX_POSITIONS listed positions of one
/// sequence store among the rows of the filter, and how often — Aggregated's group-by with sequence positions as columns.  Per
/// partition the symbol of every row at the listed positions (K16, silo_gpu_position_symbols), packed six positions to a uint32
/// id column (silo_gpu_haplotype_ids) behind the dictionary ids of the groupByFields, counted and merged over partitions by the
/// helper Aggregated uses (metadata_actions.cpp).  The symbols are the store's full alphabet: the missing symbol and ambiguity
/// codes are haplotype characters like any other, unless excludeIncomplete leaves out the rows that hold one at a listed position.
/// One row per occurring tuple: the groupByFields, haplotype (the characters in request order), count, proportion (count over the
/// sum of all counts of the response before limit and offset).  No counterpart in the reference.
template <typename SymbolType>
class Haplotypes : public Action {
  public:
   static constexpr uint32_t MAX_POSITIONS = SILO_GPU_MAX_HAPLOTYPE_POSITIONS;
   static constexpr uint32_t POSITIONS_PER_COLUMN = SILO_GPU_HAPLOTYPE_POSITIONS_PER_COLUMN;
   static constexpr uint32_t MAX_ID_COLUMNS = (MAX_POSITIONS + POSITIONS_PER_COLUMN - 1) / POSITIONS_PER_COLUMN;
   static constexpr uint32_t MAX_FIELDS = SILO_GPU_MAX_GROUP_COLUMNS - MAX_ID_COLUMNS;
   static std::string actionName() { return std::is_same_v<SymbolType, Nucleotide> ? "Haplotypes" : "AminoAcidHaplotypes"; }

   Haplotypes(std::optional<std::string> sequence_name, std::vector<uint32_t> positions, std::vector<std::string> group_by_fields, bool exclude_incomplete)
       : sequence_name(std::move(sequence_name)), positions(std::move(positions)), group_by_fields(std::move(group_by_fields)),
         exclude_incomplete(exclude_incomplete) {}

  private:
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::vector<uint32_t> positions;           // 1-based, distinct, in request order
   std::vector<std::string> group_by_fields;
   bool exclude_incomplete;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};
/// The parser of Haplotypes / AminoAcidHaplotypes (metadata_actions.cpp).
template <typename SymbolType>
std::unique_ptr<Action> parseHaplotypes(const json::Value& json);
/// Does a tuple space of these cardinalities (a column without values counts as 1) hold fewer than 2^64 - 1 tuples — the empty key
/// of the hash table of silo_gpu_group_count_hashed?  Overflow-checked (metadata_actions.cpp).
bool tupleSpaceFits(const std::vector<uint32_t>& cardinalities);

/// details.cpp: the metadata of the selected rows.  The filter runs on the device; the rows are read from the host
/// copies of the columns.
class Details : public Action {
   std::vector<std::string> fields;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   explicit Details(std::vector<std::string> fields) : fields(std::move(fields)) {}
   [[nodiscard]] QueryResult executeAndOrder(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
   [[nodiscard]] QueryResult finish(const Database& database, Pending& pending) const override;
};

/// fasta.cpp: primary key + the unaligned nucleotide sequences of the selected rows (host data only; sequence_actions.cpp).
class Fasta : public Action {
   std::vector<std::string> sequence_names;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr size_t SEQUENCE_LIMIT = 10'000;
   explicit Fasta(std::vector<std::string>&& sequence_names) : sequence_names(std::move(sequence_names)) {}
};

/// insertions.cpp: the distinct insertions of the selected rows with their counts (k_count_pairs per insertion index).
template <typename SymbolType>
class InsertionAggregation : public Action {
   std::vector<std::string> column_names;
   std::vector<std::string> sequence_names;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   InsertionAggregation(std::vector<std::string>&& column_names, std::vector<std::string>&& sequence_names)
       : column_names(std::move(column_names)), sequence_names(std::move(sequence_names)) {}
};

/// fasta_aligned.cpp: primary key + the aligned sequences of the selected rows, gathered from the planes on the
/// device (k_reconstruct_sequences; sequence_actions.cpp).
class FastaAligned : public Action {
   std::vector<std::string> sequence_names;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   explicit FastaAligned(std::vector<std::string>&& sequence_names) : sequence_names(std::move(sequence_names)) {}
};

/// MutationsPerSequence / AminoAcidMutationsPerSequence (sequence_actions.cpp): what each selected sequence carries against the
/// reference of ONE sequence store — its substitutions, its deletions and the stretches where it holds the missing symbol as maximal
/// runs, its ambiguous positions — the diff a client would otherwise make of a FastaAligned response, row by row; the row-wise dual
/// of Mutations.  The sequences are numbered in partition order, then by ascending row id, as FastaAligned returns them.  The rows
/// of every partition are gathered (silo_gpu_reconstruct_sequences) into their slice of ONE pooled [n x positions] buffer, the
/// reference is uploaded once, and ONE silo_gpu_sequence_differences (K18) runs over all n rows with room for FIRST_WORDS_PER_ROW x n
/// record words; where the total asks for more, a second one with exactly that many runs on the characters still on the device.
/// The host re-checks every fetched row before it becomes text.  One row per sequence: the primary key, sequenceName,
/// substitutions ("C241T,A23403G"), deletions and missing ("11288-11296,21991": 1-based, inclusive), ambiguous ("C1059Y") — lists
/// joined by commas, "" when empty — and substitutionCount, deletedPositions, missingPositions, ambiguousPositions.  Insertions
/// are not part of it.  No counterpart in the reference.
template <typename SymbolType>
class MutationsPerSequence : public Action {
  public:
   static constexpr uint32_t SEQUENCE_LIMIT = SILO_GPU_MAX_DIFFERENCE_ROWS;
   static constexpr uint32_t FIRST_WORDS_PER_ROW = 32;
   static std::string actionName() { return std::is_same_v<SymbolType, Nucleotide> ? "MutationsPerSequence" : "AminoAcidMutationsPerSequence"; }

   explicit MutationsPerSequence(std::optional<std::string> sequence_name) : sequence_name(std::move(sequence_name)) {}

  private:
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};
/// The parser of MutationsPerSequence / AminoAcidMutationsPerSequence (sequence_actions.cpp).
template <typename SymbolType>
std::unique_ptr<Action> parseMutationsPerSequence(const json::Value& json);

/// DistanceMatrix (distance_actions.cpp): per unordered pair of the selected sequences the positions of one aligned sequence where
/// both hold a valid mutation symbol (comparedPositions) and where those two differ (distance) — the SNP distance matrix a
/// client would otherwise compute from a FastaAligned response.  The sequences are numbered in partition order, then by
/// ascending row id; one row per pair i < j, row-major; with maxDistance only the pairs at most that far apart.  The rows
/// of every partition are gathered (silo_gpu_reconstruct_sequences) and packed into bit planes over positions
/// (silo_gpu_distance_pack) in ONE buffer, so that one pair kernel (K10, silo_gpu_distance_pairs) compares rows of different
/// partitions too, and one table is fetched per query.
class DistanceMatrix : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::optional<uint32_t> max_distance;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t SEQUENCE_LIMIT = SILO_GPU_MAX_DISTANCE_ROWS;
   DistanceMatrix(std::optional<std::string> sequence_name, std::optional<uint32_t> max_distance)
       : sequence_name(std::move(sequence_name)), max_distance(max_distance) {}
};

/// Clusters (distance_actions.cpp): the single-linkage clusters of the selected sequences — numbered as DistanceMatrix numbers them —
/// at a bound on DistanceMatrix's distance on one aligned sequence: two sequences are linked iff their distance is <= maxDistance
/// and they compare at >= minComparedPositions positions, and a cluster is a connected component of the links.  One row per
/// sequence: its key, the key of the lowest-numbered member of its cluster, the cluster's size; minClusterSize drops the rows of
/// smaller clusters.  The rows are gathered and packed in batches of SILO_GPU_MAX_DISTANCE_ROWS into ONE plane buffer; then one
/// silo_gpu_distance_within (a bit per pair, K12), one silo_gpu_adjacency_components, and n labels are fetched.
class Clusters : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   uint32_t max_distance;
   uint32_t min_compared_positions;
   uint32_t min_cluster_size;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t SEQUENCE_LIMIT = SILO_GPU_MAX_CLUSTER_ROWS;
   Clusters(std::optional<std::string> sequence_name, uint32_t max_distance, uint32_t min_compared_positions, uint32_t min_cluster_size)
       : sequence_name(std::move(sequence_name)),
         max_distance(max_distance),
         min_compared_positions(min_compared_positions),
         min_cluster_size(min_cluster_size) {}
};

/// MinimumSpanningTree (distance_actions.cpp): the minimum spanning forest of the selected sequences — numbered as DistanceMatrix
/// numbers them — over the graph whose edges are the pairs i < j with distance <= maxDistance (absent: no bound) and >=
/// minComparedPositions positions compared, ordered by the key distance * 2^26 + i * 2^13 + j.  The order is strict, so the forest is
/// unique; cut at any d it leaves the clusters of Clusters at d.  One row per edge of the forest: the two keys, the distance, the
/// compared positions, by ascending key; a sequence without an edge is in no row.  The rows are gathered and packed as for Clusters;
/// then one silo_gpu_distance_weights (the n x n matrix of the edges' distances: 4 n^2 bytes, 256 MB at the limit), one
/// silo_gpu_spanning_forest, one silo_gpu_distance_listed_pairs (K13), and ONE fetch of the count, the keys and the edges' counts.
class MinimumSpanningTree : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::optional<uint32_t> max_distance;
   uint32_t min_compared_positions;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t SEQUENCE_LIMIT = SILO_GPU_MAX_SPANNING_ROWS;
   MinimumSpanningTree(std::optional<std::string> sequence_name, std::optional<uint32_t> max_distance, uint32_t min_compared_positions)
       : sequence_name(std::move(sequence_name)), max_distance(max_distance), min_compared_positions(min_compared_positions) {}
};

/// NearestAmong (distance_actions.cpp): for every sequence the filter selects (a subject) its `neighbours` closest sequences among
/// those `among` selects (the candidates; absent: the query's own filter), by DistanceMatrix's distance on one aligned sequence.
/// Each side is numbered on its own as DistanceMatrix numbers a selection.  A candidate is eligible for a subject when it is another
/// database row, >= minComparedPositions positions are compared and the distance is <= maxDistance (absent: no bound); a subject
/// lists its lowest eligible candidates by (distance, candidate number), a strict order.  One row per (subject, listed candidate):
/// the two keys, the 1-based rank, the distance, the compared positions, by subject, then rank; a subject without an eligible
/// candidate is in no row.  Both sides are gathered and packed as for Clusters, each into its own plane buffer; then one
/// silo_gpu_distance_cross (the m x n cells: 8 m n bytes, 128 MB at the limit, which never leave the device), one
/// silo_gpu_nearest_columns (K14), and ONE fetch of the counts and the lists.
class NearestAmong : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::unique_ptr<filter_expressions::Expression> among;  // null: the query's own filter
   uint32_t neighbours;
   std::optional<uint32_t> max_distance;
   uint32_t min_compared_positions;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t SUBJECT_LIMIT = SILO_GPU_MAX_CROSS_ROWS;
   static constexpr uint32_t CANDIDATE_LIMIT = SILO_GPU_MAX_CROSS_COLUMNS;
   static constexpr uint32_t NEIGHBOUR_LIMIT = SILO_GPU_MAX_NEIGHBOUR_COLUMNS;
   static constexpr uint32_t DEFAULT_NEIGHBOURS = 1;
   NearestAmong(
      std::optional<std::string> sequence_name, std::unique_ptr<filter_expressions::Expression> among, uint32_t neighbours,
      std::optional<uint32_t> max_distance, uint32_t min_compared_positions
   )
       : sequence_name(std::move(sequence_name)),
         among(std::move(among)),
         neighbours(neighbours),
         max_distance(max_distance),
         min_compared_positions(min_compared_positions) {}
};

/// NearestNeighbours (distance_actions.cpp): the `neighbours` rows of the WHOLE database closest to one query sequence — a row named
/// by its primary key (then left out of its own list) or a literal aligned string — by DistanceMatrix's distance on one aligned
/// sequence, among the rows the filter selects and, with maxDistance, at most that far away.  Per partition one
/// silo_gpu_query_distances (every row's distance and compared positions read off the store's layout, K11) and one
/// silo_gpu_nearest_rows (the k smallest on the device); the partitions' lists are merged by (distance, partition, row).
class NearestNeighbours : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::optional<json::Value> primary_key;    // exactly one of the two
   std::optional<std::string> sequence;
   uint32_t neighbours;
   std::optional<uint32_t> max_distance;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t NEIGHBOUR_LIMIT = SILO_GPU_MAX_NEAREST_ROWS;
   static constexpr uint32_t DEFAULT_NEIGHBOURS = 10;
   NearestNeighbours(
      std::optional<std::string> sequence_name, std::optional<json::Value> primary_key, std::optional<std::string> sequence, uint32_t neighbours,
      std::optional<uint32_t> max_distance
   )
       : sequence_name(std::move(sequence_name)),
         primary_key(std::move(primary_key)),
         sequence(std::move(sequence)),
         neighbours(neighbours),
         max_distance(max_distance) {}
};

/// DistinctSequenceCounts (distance_actions.cpp; no counterpart in the reference): the largest classes of rows with equal aligned
/// sequences among the rows the filter selects — the classes of the filter expression DistinctSequences (equal 128-bit row hashes,
/// K20), each with its size and the primary key of its representative, the row DistinctSequences keeps.  Of the classes of at
/// least minCount rows the first maxClasses by (count descending, representative's row number in the database ascending), one
/// response row {count, primaryKey} each, in that order.  All on the device (K21): the owner table DistinctSelection builds
/// (operators::buildDistinctTable), silo_gpu_distinct_count and silo_gpu_distinct_classes per partition, silo_gpu_smallest_keys, and
/// one download of at most maxClasses keys.
class DistinctSequenceCounts : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   uint32_t min_count;
   uint32_t max_classes;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t CLASS_LIMIT = SILO_GPU_MAX_DISTINCT_CLASSES;
   static constexpr uint32_t DEFAULT_CLASSES = 1024;
   DistinctSequenceCounts(std::optional<std::string> sequence_name, uint32_t min_count, uint32_t max_classes)
       : sequence_name(std::move(sequence_name)), min_count(min_count), max_classes(max_classes) {}
};

/// CellCountDistribution (sequence_actions.cpp; no counterpart in the reference): the histogram of value(r) — the sum of the listed
/// kinds of row r's cell counts, as the filter expression CellCount bounds it — over the rows the filter selects.  Bin b =
/// min(value / binWidth, maxBins - 1); one response row {from, to, count} per non-empty bin, ascending; the last bin is open
/// ("to": null).  All on the device (K22): every store's kept table (silo_gpu_store_row_cell_counts), one
/// silo_gpu_cell_count_histogram per partition with selected rows into one array of bins, and one download of it.
class CellCountDistribution : public Action {
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   uint32_t kinds_mask;
   uint32_t bin_width;
   uint32_t max_bins;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

  public:
   static constexpr uint32_t BIN_LIMIT = SILO_GPU_MAX_CELL_COUNT_BINS;
   static constexpr uint32_t DEFAULT_BINS = 1024;
   CellCountDistribution(std::optional<std::string> sequence_name, uint32_t kinds_mask, uint32_t bin_width, uint32_t max_bins)
       : sequence_name(std::move(sequence_name)), kinds_mask(kinds_mask), bin_width(bin_width), max_bins(max_bins) {}
};

/// CellCountByRegion (sequence_actions.cpp; no counterpart in the reference): for each of up to 256 named regions of one aligned
/// sequence, how many of the selected rows have a number of cells of the listed kinds inside the region within the region's bounds
/// (its own, or else the action's).  One response row {region, positionFrom, positionTo, count, total} per region, in request
/// order; total is the number of selected rows.  All on the device (K23): the regions are coloured into chunks of pairwise
/// disjoint regions (colourRegions); per partition with selected rows and per chunk one silo_gpu_region_cell_values and one
/// silo_gpu_count_values into ONE array of counts, and one download of it.
class CellCountByRegion : public Action {
  public:
   struct Region {
      std::string name;
      uint32_t first, end;  // 0-based, half-open
      uint32_t at_least, at_most;
   };
   static constexpr uint32_t REGION_LIMIT = SILO_GPU_MAX_REGIONS;
   static constexpr size_t REGION_VALUE_BUDGET_BYTES = size_t{256} << 20;  // of columns per chunk, for the largest partition
   CellCountByRegion(std::optional<std::string> sequence_name, uint32_t kinds_mask, std::vector<Region> regions)
       : sequence_name(std::move(sequence_name)), kinds_mask(kinds_mask), regions(std::move(regions)) {}
   /// Chunks of indices into `ranges` ([first, end) each): sorted by start, each region goes into the first chunk in which it
   /// overlaps none and which has fewer than `max_regions` regions; within a chunk the regions ascend.  max_regions >= 1.
   static std::vector<std::vector<uint32_t>> colourRegions(const std::vector<std::pair<uint32_t, uint32_t>>& ranges, size_t max_regions);

  private:
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   uint32_t kinds_mask;
   std::vector<Region> regions;
   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

template <typename SymbolType>
class Mutations : public Action {
   std::vector<std::string> sequence_names;
   double min_proportion;

   const std::string MUTATION_FIELD_NAME = "mutation";
   const std::string SEQUENCE_FIELD_NAME = "sequenceName";
   const std::string PROPORTION_FIELD_NAME = "proportion";
   const std::string COUNT_FIELD_NAME = "count";

   struct PrefilteredBitmaps {
      std::vector<std::pair<const OperatorResult&, const SequenceStorePartition<SymbolType>&>> bitmaps;
      std::vector<std::pair<const OperatorResult&, const SequenceStorePartition<SymbolType>&>> full_bitmaps;
   };

   static std::map<std::string, PrefilteredBitmaps> preFilterBitmaps(const Database& database, std::vector<OperatorResult>& bitmap_filter);

   /// Launches the K1 scans of one sequence store into its slice counts[position][valid symbol] of the query's
   /// count table (accumulating over partitions); returns with the scans in flight on this thread's stream.
   /// min_proportion > 0: the table is read by this action's row selection alone; where ONE scan fills the store's slice, that
   /// scan may leave out escape keys that cannot reach the proportion (ScanBatcher::Request::min_proportion).
   static void calculateMutationsPerPosition(
      const Database& database, const SequenceStore<SymbolType>& sequence_store, const PrefilteredBitmaps& bitmap_filter,
      uint32_t* device_counts, double min_proportion = 0, const silo_gpu_select_sink* sink = nullptr
   );

   /// `counts` = the slice counts[position][valid symbol] of one store, on the host.
   void addMutationsToOutput(
      const std::string& sequence_name, const SequenceStore<SymbolType>& sequence_store, const uint32_t* counts,
      std::vector<QueryResultEntry>& output
   ) const;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;

   /// One row of the result from a cell the device selected.
   void addSelectedRowToOutput(
      const std::string& sequence_name, const SequenceStore<SymbolType>& sequence_store, uint32_t position, const silo_gpu_mutation_row& row,
      std::vector<QueryResultEntry>& output
   ) const;
   struct PendingScans : public Action::Pending {
      std::vector<std::string> sequence_names;  // the requested stores, in output order
      /// counts of all stores of the alphabet (MutationTableLayout), then the list written by k_mutations_select:
      /// [n_rows, -, -, -] + row_capacity rows
      DeviceBuffer device_table;
      size_t table_bytes = 0;
      uint32_t row_capacity = 0;  // 0: the host selects from the whole table
      HostFetch fetch;            // the whole table, enqueued right behind the scans (row_capacity == 0)
      RowSlot row_slot;           // the list of selected rows, written by the kernel straight into page-locked host memory
      HostFetch check_fetch;      // sharded: the two fingerprint sums behind the table (checkSameQuery)
      uint64_t fingerprint = 0;
   };
   [[nodiscard]] QueryResult collect(const Database& database, PendingScans& scans) const;
   /// A result row as the device (or the host's pass over the whole table) selects it, before any text is made.
   struct SelectedRow {
      const std::string* sequence_name;
      const SequenceStore<SymbolType>* sequence_store;
      uint32_t position;  // within the store
      uint32_t symbol_index;
      uint32_t count;
      uint32_t total;
   };
   /// The selected rows in the reference's output order: stores in request order, positions ascending, symbols in
   /// VALID_MUTATION_SYMBOLS order (mutations.cpp:190-229, 259-268).
   [[nodiscard]] std::vector<SelectedRow> collectSelected(const Database& database, PendingScans& scans) const;
   /// The selected rows as they arrive, for finishJson: position in the query's table, no particular order.  They stay in the
   /// row slot; only where the whole table had to be read (no row slot, or more rows than it holds) are they made in `from_table`.
   [[nodiscard]] std::pair<const silo_gpu_mutation_row*, size_t> deliveredRows(
      const Database& database, PendingScans& scans, std::vector<silo_gpu_mutation_row>& from_table
   ) const;

  public:
   [[nodiscard]] std::unique_ptr<Action::Pending> begin(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
   [[nodiscard]] QueryResult finish(const Database& database, Action::Pending& pending) const override;
   [[nodiscard]] std::string finishJson(const Database& database, Action::Pending& pending) const override;

   Mutations(std::vector<std::string>&& sequence_names, double min_proportion)
       : sequence_names(std::move(sequence_names)), min_proportion(min_proportion) {}
};

// ---- the count-table actions (table_actions.cpp) --------------------------------------------------------------------------
// MutationsOverTime, QueriesOverTime and CrossTabulation each fill one small uint32 table on the device, one kernel call (K7 / K8 /
// K9) per partition and batch, and fetch it once.  What they share is written once in table_actions.cpp: requireUnsharded, the
// date column (requireDateColumn, deviceDates, dateBounds, dateText), the table's life (countTable), evaluateSubFilter, and the
// LiveSet that keeps bitsets and scratch out of the pool while a launch may read them.

/// A date range of the over-time actions: both ends inclusive, none = unbounded on that side.
struct OverTimeDateRange {
   std::optional<common::Date> from;
   std::optional<common::Date> to;
};

/// Bitsets of sub-expressions QueriesOverTime and CrossTabulation (half of them per side) keep alive at a time: bounds the pool
/// memory of a partition at 64 x row_words x 8 bytes.
constexpr uint32_t MAX_LIVE_FILTERS = 64;

/// MutationsOverTime / AminoAcidMutationsOverTime: for listed mutations and date ranges, per (mutation, range) the rows of the
/// filter within the range that carry the symbol (count) and that have any valid mutation symbol at the position (coverage) —
/// the cell and the total of a Mutations table under And(filter, date in range).  Dense: every (mutation, range) is a row.
/// Both ends of a range are inclusive on every date column; NULL dates fall in no range.  One grouped count (K7) per
/// (partition, sequence store), one table fetched per query (countTable).
template <typename SymbolType>
class MutationsOverTime : public Action {
  public:
   struct Mutation {
      std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
      std::optional<char> reference_symbol;
      uint32_t position;  // 1-based
      typename SymbolType::Symbol symbol;
   };
   using DateRange = OverTimeDateRange;
   static constexpr uint32_t MAX_RANGES = SILO_GPU_MAX_DATE_RANGES;
   static constexpr uint32_t MAX_MUTATIONS = SILO_GPU_MAX_GROUPED_MUTATIONS;

   MutationsOverTime(std::vector<Mutation> mutations, std::string date_field, std::vector<DateRange> date_ranges)
       : mutations(std::move(mutations)), date_field(std::move(date_field)), date_ranges(std::move(date_ranges)) {}

  private:
   std::vector<Mutation> mutations;
   std::string date_field;
   std::vector<DateRange> date_ranges;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

/// QueriesOverTime: for labelled queries and date ranges, per (query, range) the rows of the filter within the range that match
/// the query's countQuery (count) and its coverageQuery (coverage) — what Aggregated counts under And(filter, query, date in
/// range), with both ends of a range inclusive on every date column and NULL dates in no range.  Dense: every (query, range) is a
/// row, queries outermost, in request order.  Sub-expressions with the same JSON text are evaluated and counted once per partition;
/// per partition one grouped filter count (K8) per MAX_LIVE_FILTERS bitsets (evaluateSubFilter, LiveSet), one table fetched per
/// query (countTable).
class QueriesOverTime : public Action {
  public:
   struct LabelledQuery {
      std::string display_label;
      uint32_t count_filter;     // indices into the distinct sub-expressions
      uint32_t coverage_filter;
   };
   static constexpr uint32_t MAX_RANGES = SILO_GPU_MAX_DATE_RANGES;
   static constexpr uint32_t MAX_QUERIES = 1024;
   static_assert(2 * MAX_QUERIES <= SILO_GPU_MAX_GROUPED_FILTERS && MAX_LIVE_FILTERS <= SILO_GPU_MAX_GROUPED_FILTERS);

   QueriesOverTime(
      std::vector<LabelledQuery> queries, filter_expressions::ExpressionVector filters, std::string date_field, std::vector<OverTimeDateRange> date_ranges
   )
       : queries(std::move(queries)), filters(std::move(filters)), date_field(std::move(date_field)), date_ranges(std::move(date_ranges)) {}

  private:
   std::vector<LabelledQuery> queries;
   filter_expressions::ExpressionVector filters;  // the distinct countQuery / coverageQuery expressions
   std::string date_field;
   std::vector<OverTimeDateRange> date_ranges;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

/// CrossTabulation: for two lists of labelled queries, per (row query, column query) the rows of the filter that match both —
/// what Aggregated counts under And(filter, row, column) — with the marginals And(filter, row), And(filter, column) and the rows
/// of the filter itself.  Dense: every pair is a row, row queries outermost, in request order.  No columnQueries: the row
/// queries stand on both sides (the co-occurrence matrix).  Sub-expressions with the same JSON text are parsed once and take one
/// row / column of the device table; per partition one pair count (K9) per batch of at most MAX_LIVE_FILTERS / 2 bitsets a side,
/// one table fetched per query (the same helpers of table_actions.cpp as QueriesOverTime).
class CrossTabulation : public Action {
  public:
   struct LabelledQuery {
      std::string display_label;
      uint32_t slot;  // index into its side's distinct sub-expressions: the row / column of the device table
   };
   static constexpr uint32_t MAX_QUERIES = SILO_GPU_MAX_CROSS_FILTERS;  // per list
   static constexpr uint32_t MAX_CELLS = 65536;                         // the response has one JSON row per cell
   static_assert(MAX_LIVE_FILTERS / 2 >= 2 && MAX_LIVE_FILTERS / 2 <= SILO_GPU_MAX_CROSS_FILTERS);

   CrossTabulation(
      std::vector<LabelledQuery> row_queries, std::vector<LabelledQuery> column_queries, std::vector<uint32_t> row_filters,
      std::vector<uint32_t> column_filters, filter_expressions::ExpressionVector filters
   )
       : row_queries(std::move(row_queries)),
         column_queries(std::move(column_queries)),
         row_filters(std::move(row_filters)),
         column_filters(std::move(column_filters)),
         filters(std::move(filters)) {}

  private:
   std::vector<LabelledQuery> row_queries;
   std::vector<LabelledQuery> column_queries;
   std::vector<uint32_t> row_filters;     // the distinct sub-expressions of each side (indices into filters), in order of first use
   std::vector<uint32_t> column_filters;
   filter_expressions::ExpressionVector filters;  // the distinct sub-expressions of both lists

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

/// Consensus / AminoAcidConsensus: the consensus sequence of one sequence store over the rows of the query's filter, or over each of
/// up to MAX_GROUPS named groups — the filter AND the group's own expression, per partition.  Per group and position the counts of
/// the valid mutation symbols (a cell of a Mutations table) and their sum, the depth: below min_depth the missing symbol (low
/// coverage); otherwise the symbols, by descending count, up to the one at which they reach ceil(depth * threshold), with every
/// symbol tied with that one — a single symbol as itself ('-': deleted), several as the IUPAC code of the set (nucleotides, 'N' with
/// '-' among them) or 'X' (amino acids): ambiguous.  One row per group, in request order: name (null without groups), sequenceName,
/// count, consensus, ambiguousPositions, lowCoveragePositions, deletedPositions, differences (unambiguous, covered calls that are
/// not the reference's symbol).  Per partition the exact Mutations scan of all groups' bitsets (silo_gpu_mutations_scan_batch: a
/// pass over the planes per SILO_GPU_MAX_SCAN_BATCH groups) accumulates into one table per group; one consensus call (K15) and one
/// fetch of characters and sums: the tables never leave the device.  No counterpart in the reference.
template <typename SymbolType>
class Consensus : public Action {
  public:
   struct Group {
      std::optional<std::string> name;                          // none: the one group of a request without groups
      std::unique_ptr<filter_expressions::Expression> filter;  // null: the query's filter alone
   };
   static constexpr uint32_t MAX_GROUPS = SILO_GPU_MAX_CONSENSUS_TABLES;
   static constexpr double DEFAULT_THRESHOLD = 0.5;
   static constexpr uint32_t DEFAULT_MIN_DEPTH = 1;
   static_assert(MAX_GROUPS <= MAX_LIVE_FILTERS);  // the bitsets of every group of a partition are alive at a time
   static std::string actionName() { return std::is_same_v<SymbolType, Nucleotide> ? "Consensus" : "AminoAcidConsensus"; }

   Consensus(std::optional<std::string> sequence_name, std::vector<Group> groups, double threshold, uint32_t min_depth)
       : sequence_name(std::move(sequence_name)), groups(std::move(groups)), threshold(threshold), min_depth(min_depth) {}

  private:
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::vector<Group> groups;
   double threshold;
   uint32_t min_depth;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

/// MutationsComparison / AminoAcidMutationsComparison: how often each of 2 .. MAX_GROUPS named groups — the query's filter AND the
/// group's own expression, per partition, as Consensus resolves them — carries each mutation of one sequence store that any of them
/// carries.  With c a cell of a group's Mutations table and cov the sum of the cells of its position: a group passes (position,
/// symbol) iff cov > 0 and c > the bound of Mutations' row selection at min_proportion; difference = the highest minus the lowest
/// c / cov over the groups with cov > 0 (0.0 with fewer than two); a mutation is selected iff the symbol is not the reference's, some
/// group passes it and difference >= min_difference.  One row per selected mutation and group, in the order position, symbol, group
/// of the request: mutation, sequenceName, position (1-based), group, count, coverage, proportion (null where coverage is 0),
/// difference (the same on the rows of a mutation).  Per partition the exact Mutations scan of all groups' bitsets into one table per
/// group, as for Consensus; one comparison (K17, silo_gpu_mutations_compare) with room for FIRST_CAPACITY records, a second one with
/// exactly as much room as the first one's counter asks for where that is more; the header and the records with their cells are
/// fetched: the tables never leave the device.  Every record is checked against the rule before it becomes rows.  No counterpart in
/// the reference.
template <typename SymbolType>
class MutationsComparison : public Action {
  public:
   struct Group {
      std::string name;
      std::unique_ptr<filter_expressions::Expression> filter;
   };
   static constexpr uint32_t MIN_GROUPS = 2;
   static constexpr uint32_t MAX_GROUPS = SILO_GPU_MAX_COMPARISON_TABLES;
   static constexpr double DEFAULT_MIN_PROPORTION = 0.05;
   static constexpr double DEFAULT_MIN_DIFFERENCE = 0;
   static constexpr uint32_t FIRST_CAPACITY = 1024;  // records of the first comparison: a response above it costs a second launch
   static_assert(MAX_GROUPS <= MAX_LIVE_FILTERS);    // the bitsets of every group of a partition are alive at a time
   static std::string actionName() { return std::is_same_v<SymbolType, Nucleotide> ? "MutationsComparison" : "AminoAcidMutationsComparison"; }

   MutationsComparison(std::optional<std::string> sequence_name, std::vector<Group> groups, double min_proportion, double min_difference)
       : sequence_name(std::move(sequence_name)), groups(std::move(groups)), min_proportion(min_proportion), min_difference(min_difference) {}

  private:
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::vector<Group> groups;
   double min_proportion;
   double min_difference;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

/// MeanDistances / AminoAcidMeanDistances: the sums of DistanceMatrix's `distance` and `compared` (a position counts when both rows
/// hold a valid mutation symbol) over every pair of rows within each and between every two of 1 .. MAX_GROUPS groups — the query's
/// filter AND the group's own expression, per partition, as Consensus resolves them; without groups the filter alone — in each of
/// 1 .. MAX_REGIONS named regions of one sequence store (without regions the whole sequence), for groups of any size: no row is
/// compared with a row.  With c a cell of a group's Mutations table and cov the sum of the cells of its position, the pairs of a row
/// of g and a row of h that differ at the position are cov_g cov_h - sum_s c_g c_h and those compared cov_g cov_h; within a group
/// (cov^2 - sum_s c^2) / 2 and cov (cov - 1) / 2, the unordered pairs.  One row per region and pair g <= h (g == h only when
/// `between` is false), in the order region, g, h of the request: region, positionFrom, positionTo (1-based, inclusive), sequenceName,
/// group, otherGroup, count, otherCount, pairs (n_g n_h, or n (n - 1) / 2), differences, comparedPositions (the three as decimal
/// strings: they pass 2^53), segregatingSites (g == h: positions with two symbols; else null), fixedDifferences (g < h: positions
/// where both are covered and share no symbol; else null), meanDistance = differences / pairs, meanCompared = comparedPositions /
/// pairs, distancePerSite = differences / comparedPositions (each the correctly rounded doubles of the integers, one IEEE division;
/// null where the divisor is 0).  A row that lies in both g and h forms a pair with itself between them: distance 0, compared.  The
/// exact Mutations scan of all groups into one table per group, as for Consensus; one call of K24 (silo_gpu_table_pair_sums) and one
/// fetch of the records: the tables never leave the device.  Every record is checked before it becomes a row.  No counterpart in the
/// reference.
template <typename SymbolType>
class MeanDistances : public Action {
  public:
   struct Group {
      std::optional<std::string> name;                          // none: the one group of a request without groups
      std::unique_ptr<filter_expressions::Expression> filter;  // null: the query's filter alone
   };
   struct Region {
      std::optional<std::string> name;  // none: the one region of a request without regions, the whole sequence
      uint32_t first = 0;               // 0-based
      uint32_t end = 0;                 // past the last position; of the unnamed region: the sequence's length, known at execute
   };
   static constexpr uint32_t MAX_GROUPS = SILO_GPU_MAX_PAIR_SUM_TABLES;
   static constexpr uint32_t MAX_REGIONS = SILO_GPU_MAX_PAIR_SUM_RANGES;
   static constexpr size_t MAX_ROWS = 65536;       // of a response before limit and offset
   static_assert(MAX_GROUPS <= MAX_LIVE_FILTERS);  // the bitsets of every group of a partition are alive at a time
   static std::string actionName() { return std::is_same_v<SymbolType, Nucleotide> ? "MeanDistances" : "AminoAcidMeanDistances"; }

   MeanDistances(std::optional<std::string> sequence_name, std::vector<Group> groups, std::vector<Region> regions, bool between)
       : sequence_name(std::move(sequence_name)), groups(std::move(groups)), regions(std::move(regions)), between(between) {}

  private:
   std::optional<std::string> sequence_name;  // none: the default nucleotide sequence
   std::vector<Group> groups;
   std::vector<Region> regions;
   bool between;

   void validateOrderByFields(const Database& database) const override;
   [[nodiscard]] QueryResult execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const override;
};

}  // namespace actions

class Query {
  public:
   std::unique_ptr<filter_expressions::Expression> filter;
   std::unique_ptr<actions::Action> action;
   explicit Query(const std::string& query_string);
};

class QueryEngine {
  private:
   const Database& database;

  public:
   explicit QueryEngine(const Database& database) : database(database) {}
   virtual ~QueryEngine() = default;
   [[nodiscard]] virtual QueryResult executeQuery(const std::string& query) const;
   /// executeQuery as the response body (the bytes of toJsonText(executeQuery(query))): what a caller that only forwards
   /// the JSON — silo_api's QueryHandler::post, query_handler.cpp:38-41 — needs, without the QueryResult rows in between.
   [[nodiscard]] std::string executeQueryJson(const std::string& query) const;

   /// Outcome of one query of a batch: a result, or the exception it raised (mapped to 400 / 500 by the caller
   /// exactly as for a single query, silo_api/query_handler.cpp:42-73).
   struct BatchOutcome {
      QueryResult result;
      std::string json;  // the response body, when executeQueries was asked to render it (while later queries' scans still run)
      std::exception_ptr error;
   };
   /// Executes a batch of independent queries: filters are evaluated per query, then the Mutations scans of all
   /// queries that read the same sequence store are issued together, several filters per pass over the planes.
   [[nodiscard]] std::vector<BatchOutcome> executeQueries(const std::vector<std::string>& queries, bool render_json = false) const;
};

}  // namespace query_engine
}  // namespace silo
