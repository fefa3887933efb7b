// operators.cpp — physical operators and their lowering to the fused bit-program (K3).
// Reference: src/silo/query_engine/operators/*.cpp, src/silo/query_engine/operator_result.cpp.
#include <algorithm>
#include <bit>
#include <deque>
#include <mutex>
#include <shared_mutex>

#include "query_engine.h"

namespace silo::query_engine {

// ---- OperatorResult ----------------------------------------------------------------------------
struct OperatorResult::State {
   RowSpace rows;
   std::unique_ptr<operators::Operator> root;
   std::mutex mutex;
   DeviceBuffer bitset;
   std::optional<uint32_t> count;
   const uint64_t* borrowed = nullptr;  // IndexScan roots need no kernel for the bitset
};

OperatorResult::OperatorResult(RowSpace rows, std::unique_ptr<operators::Operator> root) : state(std::make_shared<State>()) {
   state->rows = rows;
   state->root = std::move(root);
}

const RowSpace& OperatorResult::rows() const {
   return state->rows;
}

namespace {

constexpr size_t COUNT_BYTES = SILO_GPU_COUNT_SHARDS * sizeof(uint64_t);

DeviceBuffer zeroedCounter(const DatabasePartition& partition) {
   DeviceBuffer counter = partition.pool.acquire(COUNT_BYTES);
   checkGpu(silo_gpu_memset_async(counter.get(), 0, COUNT_BYTES, queryStream()), "silo_gpu_memset_async");
   return counter;
}

uint32_t readCount(const DeviceBuffer& counter) {
   uint64_t shards[SILO_GPU_COUNT_SHARDS];
   checkGpu(silo_gpu_memcpy_d2h(shards, counter.get(), COUNT_BYTES, queryStream()), "silo_gpu_memcpy_d2h");
   uint64_t total = 0;
   for (const uint64_t shard : shards) {
      total += shard;
   }
   return static_cast<uint32_t>(total);
}

bool isLeafOperand(uint32_t operand) {
   return operand >= SILO_GPU_LEAF_OPERAND;
}

/// allocRun() found no free run of slots.  ProgramBuilder::lowerChild takes the child it was lowering out of the program
/// again and evaluates it on its own; anywhere else this is a bug of the size estimates.
struct SlotsExhausted : QueryCompilationException {
   SlotsExhausted() : QueryCompilationException("Internal error: the filter program ran out of device slots") {}
};

}  // namespace

void OperatorResult::materialize() const {
   const std::lock_guard<std::mutex> lock(state->mutex);
   if ((state->bitset || state->borrowed != nullptr) && state->count.has_value()) {
      return;
   }
   const DatabasePartition& partition = *state->rows.partition;
   const size_t row_bytes = static_cast<size_t>(partition.rowWords()) * sizeof(uint64_t);
   const auto* scan = state->root->type() == operators::INDEX_SCAN ? dynamic_cast<const operators::IndexScan*>(state->root.get()) : nullptr;
   if (scan != nullptr && !scan->sparse) {
      state->borrowed = scan->bitmap;  // index_scan.cpp:28-30: borrow, no copy
      if (scan->received == nullptr) {  // a stored bitmap (not a plane received from another rank): its cardinality is kept
         const std::shared_lock<std::shared_mutex> lock(partition.cardinality_cache_mutex);
         const auto known = partition.cardinality_cache.find(scan->bitmap);
         if (known != partition.cardinality_cache.end()) {
            state->count = known->second;
            return;
         }
      }
      DeviceBuffer counter = zeroedCounter(partition);
      checkGpu(silo_gpu_popcount(partition.store, scan->bitmap, counter.as<uint64_t>(), queryStream()), "silo_gpu_popcount");
      state->count = readCount(counter);
      if (scan->received == nullptr) {
         const std::unique_lock<std::shared_mutex> lock(partition.cardinality_cache_mutex);
         if (partition.cardinality_cache.size() < (size_t{1} << 20)) {
            partition.cardinality_cache.emplace(scan->bitmap, *state->count);
         }
      }
   } else {
      DeviceBuffer out = partition.pool.acquire(row_bytes);
      ProgramBuilder builder(state->rows);
      const uint32_t slot = state->root->lower(builder);
      state->count = builder.runCounting(slot, out.as<uint64_t>(), queryStream());
      state->bitset = std::move(out);
   }
}

uint32_t OperatorResult::cardinality() const {
   {
      const std::lock_guard<std::mutex> lock(state->mutex);
      if (state->count.has_value()) {
         return *state->count;
      }
      // count-only launch: no bitset is written (Aggregated never needs it)
      if (state->root->type() == operators::EMPTY) {
         state->count = 0;
         return 0;
      }
      if (state->root->type() == operators::FULL) {
         state->count = state->rows.row_count;
         return *state->count;
      }
      const auto* scan = state->root->type() == operators::INDEX_SCAN ? dynamic_cast<const operators::IndexScan*>(state->root.get()) : nullptr;
      const bool stored = scan != nullptr && !scan->sparse && scan->received == nullptr;
      const DatabasePartition& partition = *state->rows.partition;
      if (stored) {  // the kept cardinality of a stored bitmap (see DatabasePartition::cardinality_cache)
         const std::shared_lock<std::shared_mutex> lock(partition.cardinality_cache_mutex);
         const auto known = partition.cardinality_cache.find(scan->bitmap);
         if (known != partition.cardinality_cache.end()) {
            state->count = known->second;
            return *state->count;
         }
      }
      ProgramBuilder builder(state->rows);
      const uint32_t slot = state->root->lower(builder);
      state->count = builder.runCounting(slot, nullptr, queryStream());
      if (stored) {
         const std::unique_lock<std::shared_mutex> lock(partition.cardinality_cache_mutex);
         if (partition.cardinality_cache.size() < (size_t{1} << 20)) {
            partition.cardinality_cache.emplace(scan->bitmap, *state->count);
         }
      }
      return *state->count;
   }
}

bool OperatorResult::prepareCount(ProgramBuilder& builder, silo_gpu_bitprog& program) const {
   const std::lock_guard<std::mutex> lock(state->mutex);
   if (state->count.has_value()) {
      return false;
   }
   if (state->root->type() == operators::EMPTY || state->root->type() == operators::FULL) {
      state->count = state->root->type() == operators::EMPTY ? 0 : state->rows.row_count;
      return false;
   }
   program = builder.finishProgram(state->root->lower(builder));
   return true;
}

void OperatorResult::setCount(uint32_t count) const {
   const std::lock_guard<std::mutex> lock(state->mutex);
   state->count = count;
}

const uint64_t* OperatorResult::bitset() const {
   materialize();
   return state->borrowed != nullptr ? state->borrowed : state->bitset.as<uint64_t>();
}

bool OperatorResult::isFull() const {
   return cardinality() == state->rows.row_count;
}

// ---- ProgramBuilder ----------------------------------------------------------------------------
uint32_t ProgramBuilder::allocRun(uint32_t count) {
   for (uint32_t first = 0; first + count <= SILO_GPU_MAX_SLOTS; ++first) {
      const uint32_t mask = (count == 32 ? 0xFFFFFFFFu : ((1u << count) - 1u)) << first;
      if ((used_slots & mask) == 0) {
         used_slots |= mask;
         high_water = std::max(high_water, first + count);
         return first;
      }
   }
   throw SlotsExhausted();
}

uint32_t ProgramBuilder::allocSlot() {
   return allocRun(1);
}

void ProgramBuilder::freeRun(uint32_t slot, uint32_t count) {
   const uint32_t mask = (count == 32 ? 0xFFFFFFFFu : ((1u << count) - 1u)) << slot;
   used_slots &= ~mask;
}

void ProgramBuilder::freeSlot(uint32_t slot) {
   if (!isLeafOperand(slot)) {  // leaf operands are not allocated
      freeRun(slot, 1);
   }
}

void ProgramBuilder::emit(uint32_t op, uint32_t dst, uint32_t a, uint32_t b, uint32_t imm) {
   code.push_back(op | (dst << 8) | (a << 16) | (b << 24));
   code.push_back(imm);
}

uint32_t ProgramBuilder::leaf(const uint64_t* device_bitset) {
   const auto found = std::find(leaves.begin(), leaves.end(), device_bitset);
   if (found != leaves.end()) {
      return static_cast<uint32_t>(found - leaves.begin());
   }
   leaves.push_back(device_bitset);
   return static_cast<uint32_t>(leaves.size() - 1);
}

uint32_t ProgramBuilder::sparseLeaf(uint32_t seqstore_id, uint32_t position, uint32_t symbol) {
   return leaf(sparsePointer(seqstore_id, position, symbol));
}

uint32_t ProgramBuilder::leafRun(const std::vector<const uint64_t*>& columns) {
   if (leaves.size() + columns.size() > SILO_GPU_MAX_LEAVES) {  // the callers cut their runs to what is left
      throw QueryCompilationException("Internal error: a run of stored columns does not fit the leaves of the filter program");
   }
   const auto first = static_cast<uint32_t>(leaves.size());
   leaves.insert(leaves.end(), columns.begin(), columns.end());  // consecutive, not de-duplicated
   return first | (static_cast<uint32_t>(columns.size()) << 16);
}

ProgramBuilder::Split ProgramBuilder::split(const operators::OperatorVector& children) {
   Split out;
   for (const auto& child : children) {
      if (const uint64_t* column = child->storedColumn(*this); column != nullptr) {
         out.columns.push_back(column);
      } else {
         out.composite.push_back(child.get());
      }
   }
   return out;
}

const uint64_t* ProgramBuilder::sparsePointer(uint32_t seqstore_id, uint32_t position, uint32_t symbol) {
   // Sparse planes are immutable once the store is finalised, so a materialised plane is kept for later
   // queries (bounded: beyond the budget a plane is built into a pooled temporary for this launch only).
   const DatabasePartition& partition = *rows.partition;
   const size_t row_bytes = static_cast<size_t>(partition.rowWords()) * sizeof(uint64_t);
   const uint64_t key = (static_cast<uint64_t>(seqstore_id) << 40) | (static_cast<uint64_t>(position) << 8) | symbol;
   {
      const std::shared_lock<std::shared_mutex> lock(partition.sparse_cache_mutex);
      const auto found = partition.sparse_cache.find(key);
      if (found != partition.sparse_cache.end()) {
         return found->second.as<uint64_t>();
      }
   }
   DeviceBuffer buffer = partition.pool.acquire(row_bytes);
   checkGpu(
      silo_gpu_store_sparse_plane(partition.store, seqstore_id, position, symbol, buffer.as<uint64_t>(), queryStream()),
      "silo_gpu_store_sparse_plane"
   );
   const uint64_t* pointer = buffer.as<uint64_t>();
   // other threads (on their own streams) may pick the plane up from the cache at once: finish it first
   checkGpu(silo_gpu_stream_synchronize(queryStream()), "silo_gpu_stream_synchronize");
   {
      const std::unique_lock<std::shared_mutex> lock(partition.sparse_cache_mutex);
      if ((partition.sparse_cache.size() + 1) * row_bytes <= DatabasePartition::SPARSE_CACHE_BYTES &&
          partition.sparse_cache.find(key) == partition.sparse_cache.end()) {
         partition.sparse_cache.emplace(key, std::move(buffer));
         return pointer;
      }
   }
   temporaries.push_back(std::move(buffer));
   return pointer;
}

void* ProgramBuilder::temporaryBuffer(size_t bytes) {
   DeviceBuffer buffer = rows.partition->pool.acquire(bytes);
   void* pointer = buffer.get();
   temporaries.push_back(std::move(buffer));
   buffer_stream = queryStream();
   has_buffers = true;
   return pointer;
}

void ProgramBuilder::keep(OperatorResult result) {
   materialized_children.push_back(std::move(result));
   buffer_stream = queryStream();
   has_buffers = true;
}

ProgramBuilder::~ProgramBuilder() {
   if (has_buffers) {
      (void)silo_gpu_stream_synchronize(buffer_stream);
   }
}

uint64_t* ProgramBuilder::temporaryBitset() {
   const DatabasePartition& partition = *rows.partition;
   DeviceBuffer buffer = partition.pool.acquire(static_cast<size_t>(partition.rowWords()) * sizeof(uint64_t));
   auto* pointer = buffer.as<uint64_t>();
   temporaries.push_back(std::move(buffer));
   return pointer;
}

bool ProgramBuilder::fits(const operators::Cost& cost) const {
   return code.size() / 2 + cost.instructions + 8 <= SILO_GPU_MAX_INSTRUCTIONS && leaves.size() + cost.leaves + 1 <= SILO_GPU_MAX_LEAVES &&
          static_cast<uint32_t>(std::popcount(used_slots)) + cost.slots + 1 <= SILO_GPU_MAX_SLOTS;
}

bool ProgramBuilder::hasRoom(uint32_t more_leaves, uint32_t more_instructions) const {
   return leaves.size() + more_leaves <= SILO_GPU_MAX_LEAVES && code.size() / 2 + more_instructions + 1 <= SILO_GPU_MAX_INSTRUCTIONS;
}

size_t ProgramBuilder::leafRoom() const {
   return SILO_GPU_MAX_LEAVES - leaves.size();
}

uint32_t ProgramBuilder::lowerChild(const operators::Operator& child) {
   return lowerChild(child, child.cost());
}

uint32_t ProgramBuilder::lowerChild(const operators::Operator& child, const operators::Cost& cost) {
   if (fits(cost)) {
      const size_t code_size = code.size();
      const size_t leaf_count = leaves.size();
      const uint32_t slots = used_slots;
      const uint32_t water = high_water;
      try {
         return child.lower(*this);
      } catch (const SlotsExhausted&) {
         // Cost::slots counts live slots; first-fit runs can leave holes between them.  Take back what the child emitted and
         // give it a program of its own.  The child is lowered a second time there: launches that its first lowering queued
         // (metadata comparisons, leaves fetched from other ranks) are issued again, their buffers stay with this builder.
         code.resize(code_size);
         leaves.resize(leaf_count);
         used_slots = slots;
         high_water = water;
      }
   }
   // a program of its own, whose root cuts itself into as many programs as it needs
   OperatorResult result = child.evaluate();
   const uint32_t operand = SILO_GPU_LEAF_OPERAND + leaf(result.bitset());
   materialized_children.push_back(std::move(result));
   return operand;
}

void ProgramBuilder::restart() {
   code.clear();
   leaves.clear();
   used_slots = 0;
   high_water = 0;
}

uint32_t ProgramBuilder::flush(uint32_t operand) {
   if (operand == NO_OPERAND) {
      throw QueryCompilationException("Internal error: a filter program is full before it holds a value");
   }
   uint64_t* partial = temporaryBitset();
   run(operand, partial, nullptr, queryStream());  // waits for the launch: the code and leaf arrays are written again at once
   restart();
   return SILO_GPU_LEAF_OPERAND + leaf(partial);
}

std::vector<const uint64_t*> ProgramBuilder::flushPlanes(uint32_t first, uint32_t planes) {
   std::vector<const uint64_t*> partial;
   const size_t code_size = code.size();
   for (uint32_t plane = 0; plane < planes; ++plane) {
      uint64_t* bitset = temporaryBitset();
      run(first + plane, bitset, nullptr, queryStream());
      code.resize(code_size);  // without the MOV of this plane
      partial.push_back(bitset);
   }
   restart();
   return partial;
}

void ProgramBuilder::combine(uint32_t& acc, uint32_t op, uint32_t operand) {
   if (acc == NO_OPERAND) {
      acc = operand;
      return;
   }
   const uint32_t dst = isLeafOperand(acc) ? (isLeafOperand(operand) ? allocSlot() : operand) : acc;
   emit(op, dst, acc, operand);
   if (dst != operand) {
      freeSlot(operand);
   }
   acc = dst;
}

void ProgramBuilder::foldColumns(uint32_t& acc, uint32_t fold_n, uint32_t op, const std::vector<const uint64_t*>& columns, bool may_flush) {
   for (size_t done = 0; done < columns.size();) {
      size_t take = columns.size() - done;
      if (may_flush) {
         if (!hasRoom(take >= 2 ? 2 : 1, 2)) {
            acc = flush(acc);
         }
         take = std::min(take, leafRoom());
      }
      if (take == 1) {
         combine(acc, op, SILO_GPU_LEAF_OPERAND + leaf(columns[done]));
      } else {
         const uint32_t folded = allocSlot();
         emit(fold_n, folded, 0, 0, leafRun({columns.begin() + static_cast<ptrdiff_t>(done), columns.begin() + static_cast<ptrdiff_t>(done + take)}));
         combine(acc, op, folded);
      }
      done += take;
   }
}

uint32_t ProgramBuilder::lowerChildBeside(uint32_t& acc, const operators::Operator& child, bool may_flush) {
   const operators::Cost cost = child.cost();
   if (may_flush && acc != NO_OPERAND && !code.empty() && !fits(cost)) {
      acc = flush(acc);
   }
   return lowerChild(child, cost);
}

silo_gpu_bitprog ProgramBuilder::finishProgram(uint32_t result_slot) {
   if (result_slot != 0) {
      emit(SILO_GPU_OP_MOV, 0, result_slot);
      high_water = std::max(high_water, 1u);
   }
   if (code.size() / 2 > SILO_GPU_MAX_INSTRUCTIONS || leaves.size() > SILO_GPU_MAX_LEAVES) {  // every lowering keeps to what is left
      throw QueryCompilationException("Internal error: a filter program outgrew the device limits");
   }
   silo_gpu_bitprog program{};
   program.n_instructions = static_cast<uint32_t>(code.size() / 2);
   program.code = code.data();
   program.n_leaves = static_cast<uint32_t>(leaves.size());
   program.leaves = leaves.data();
   program.n_slots = std::max(high_water, 1u);
   return program;
}

void ProgramBuilder::run(uint32_t result_slot, uint64_t* out_bitset, uint64_t* out_count, void* stream) {
   const silo_gpu_bitprog program = finishProgram(result_slot);
   checkGpu(silo_gpu_filter_eval(rows.partition->store, &program, out_bitset, out_count, stream), "silo_gpu_filter_eval");
   if (!temporaries.empty() || !materialized_children.empty()) {
      // temporaries go back to the pool when the builder dies: make sure the kernel is done with them
      checkGpu(silo_gpu_stream_synchronize(stream), "silo_gpu_stream_synchronize");
      has_buffers = has_buffers && stream != buffer_stream;
   }
}

namespace {
/// One count slot per host thread (a slot serves one launch at a time).  Never destroyed: thread exit may come
/// after the HIP runtime has shut down.
silo_gpu_count_slot* threadCountSlot() {
   thread_local silo_gpu_count_slot* slot = nullptr;
   if (slot == nullptr) {
      checkGpu(silo_gpu_count_slot_create(&slot), "silo_gpu_count_slot_create");
   }
   return slot;
}
}  // namespace

uint32_t ProgramBuilder::runCounting(uint32_t result_slot, uint64_t* out_bitset, void* stream) {
   const silo_gpu_bitprog program = finishProgram(result_slot);
   silo_gpu_count_slot* slot = threadCountSlot();
   checkGpu(silo_gpu_filter_eval_count(rows.partition->store, &program, out_bitset, slot, stream), "silo_gpu_filter_eval_count");
   uint64_t count = 0;
   // the total arrives when the last block is done: every block has read its leaves by then, so the temporaries of
   // this builder may go back to the pool without a stream synchronisation
   checkGpu(silo_gpu_count_slot_wait(slot, &count, stream), "silo_gpu_count_slot_wait");
   has_buffers = has_buffers && stream != buffer_stream;  // what wrote and read them ran ahead of the program on that stream
   return static_cast<uint32_t>(count);
}

namespace operators {

OperatorResult Operator::evaluate() const {
   return OperatorResult(rows, copy());
}

OperatorResult Operator::evaluate(std::unique_ptr<Operator> root) {
   const RowSpace rows = root->rows;
   return OperatorResult(rows, std::move(root));
}

namespace {

OperatorVector copyAll(const OperatorVector& source) {
   OperatorVector out;
   out.reserve(source.size());
   for (const auto& child : source) {
      out.push_back(child->copy());
   }
   return out;
}

/// Instructions and leaves of the children of an n-ary node (one combining instruction per child, two per negated one), and the
/// slots of a fold of them: the accumulator, once two leaf operands or a composite child have made it a slot, beside the child
/// that is being lowered.  (Threshold keeps a counter instead and takes `widest_child`.)
struct FoldCost {
   Cost total;
   uint32_t widest_child = 0;
};

FoldCost sumCost(const OperatorVector& a, const OperatorVector* b = nullptr) {
   FoldCost out;
   bool accumulator = false;  // whether the fold's value sits in a slot by now
   // One pass over the children of one sign.  Their leaf operands are taken as if they all came first (never too few slots):
   // `leaf_fold` of them put the accumulator into a slot, which costs `leaf_slots` beside it.
   const auto add = [&](const OperatorVector& children, uint32_t combining, uint32_t leaf_fold, uint32_t leaf_slots) {
      uint32_t leaf_operands = 0;
      uint32_t first = 0;  // the slots of the first child whose value arrives in a slot, and of the widest after it
      uint32_t later = 0;
      for (const auto& child : children) {
         const Cost c = child->cost();
         out.total.instructions += c.instructions + combining;
         out.total.leaves += c.leaves;
         out.widest_child = std::max(out.widest_child, c.slots);
         if (c.slots == 0) {
            ++leaf_operands;
         } else if (first == 0) {
            first = c.slots;
         } else {
            later = std::max(later, c.slots);
         }
      }
      if (leaf_operands >= leaf_fold) {
         out.total.slots = std::max(out.total.slots, (accumulator ? 1u : 0u) + leaf_slots);
         accumulator = true;
      }
      if (first != 0) {
         out.total.slots = std::max({out.total.slots, (accumulator ? 1u : 0u) + first, later == 0 ? 0u : 1u + later});
         accumulator = true;
      }
   };
   add(a, 1, 2, 1);  // two leaf operands fold into one slot
   if (b != nullptr) {
      add(*b, 2, 1, 1);  // the OR_N of the negated columns, or the slot that ANDNOT of two leaf operands needs
   }
   return out;
}

}  // namespace

// ---- Empty / Full (empty.cpp, full.cpp:24-28) ---------------------------------------------------
std::unique_ptr<Operator> Empty::copy() const {
   return std::make_unique<Empty>(rows);
}
std::unique_ptr<Operator> Empty::negate() const {
   return std::make_unique<Full>(rows);
}
uint32_t Empty::lower(ProgramBuilder& builder) const {
   const uint32_t slot = builder.allocSlot();
   builder.emit(SILO_GPU_OP_ZERO, slot);
   return slot;
}

std::unique_ptr<Operator> Full::copy() const {
   return std::make_unique<Full>(rows);
}
std::unique_ptr<Operator> Full::negate() const {
   return std::make_unique<Empty>(rows);
}
uint32_t Full::lower(ProgramBuilder& builder) const {
   const uint32_t slot = builder.allocSlot();
   builder.emit(SILO_GPU_OP_ONES, slot);
   return slot;
}

// ---- IndexScan (index_scan.cpp:28-30) -----------------------------------------------------------
std::unique_ptr<Operator> IndexScan::copy() const {
   if (sparse) {
      return std::make_unique<IndexScan>(seqstore_id, position, symbol, rows);
   }
   auto copied = std::make_unique<IndexScan>(bitmap, rows);
   copied->received = received;
   return copied;
}
std::unique_ptr<Operator> IndexScan::negate() const {
   return std::make_unique<Complement>(copy(), rows);
}
const uint64_t* IndexScan::storedColumn(ProgramBuilder& builder) const {
   return sparse ? builder.sparsePointer(seqstore_id, position, symbol) : bitmap;
}
uint32_t IndexScan::lower(ProgramBuilder& builder) const {
   // a leaf operand: the kernel stages every leaf in LDS up front, no instruction is emitted here
   const uint32_t index = sparse ? builder.sparseLeaf(seqstore_id, position, symbol) : builder.leaf(bitmap);
   return SILO_GPU_LEAF_OPERAND + index;
}

// ---- Selection (selection.cpp) ---------------------------------------------------------------------
Predicate Predicate::negated() const {  // selection.cpp:195-220: NOT (x >= v) becomes x < v — not the same for a NaN row
   static constexpr int NEGATED[] = {
      SILO_GPU_CMP_NOT_EQUALS, SILO_GPU_CMP_EQUALS, SILO_GPU_CMP_HIGHER_OR_EQUALS, SILO_GPU_CMP_LESS, SILO_GPU_CMP_LESS_OR_EQUALS,
      SILO_GPU_CMP_HIGHER};
   Predicate out = *this;
   out.comparator = NEGATED[comparator];
   return out;
}

std::unique_ptr<Operator> Selection::copy() const {
   return std::make_unique<Selection>(child != nullptr ? child->copy() : nullptr, predicates, rows);
}

std::unique_ptr<Operator> Selection::negate() const {  // selection.cpp:125-130
   if (child == nullptr && predicates.size() == 1) {
      return std::make_unique<Selection>(std::vector<Predicate>{predicates.at(0).negated()}, rows);
   }
   return std::make_unique<Complement>(this->copy(), rows);
}

Cost Selection::cost() const {
   const uint32_t accumulator = predicates.size() >= 2 ? 1 : 0;
   Cost total{static_cast<uint32_t>(predicates.size()) + 1, static_cast<uint32_t>(predicates.size()), std::max(accumulator, predicates.empty() ? 1u : 0u)};
   if (child != nullptr) {
      const Cost child_cost = child->cost();
      total.instructions += child_cost.instructions;
      total.leaves += child_cost.leaves;
      total.slots = accumulator + std::max(child_cost.slots, 1u);
   }
   return total;
}

uint32_t Selection::lower(ProgramBuilder& builder) const {
   // The reference probes every predicate row by row (selection.cpp:88-108).  Here each predicate is one pass of
   // k_bitset_from_compare over its column (4-8 bytes per row, on the query's stream, ahead of the fused program),
   // and the program ANDs the resulting bitsets like any other stored columns.
   const bool may_flush = builder.empty();
   std::vector<const uint64_t*> columns;
   for (const Predicate& predicate : predicates) {
      uint64_t* bitset = builder.temporaryBitset();
      checkGpu(
         silo_gpu_bitset_from_compare(
            rows.partition->store, bitset, predicate.column->deviceValues(), predicate.column->deviceValueType(), predicate.comparator,
            &predicate.value, queryStream()
         ),
         "silo_gpu_bitset_from_compare"
      );
      columns.push_back(bitset);
   }
   uint32_t acc = ProgramBuilder::NO_OPERAND;
   builder.foldColumns(acc, SILO_GPU_OP_AND_N, SILO_GPU_OP_AND, columns, may_flush);
   if (child != nullptr) {
      const uint32_t operand = builder.lowerChildBeside(acc, *child, may_flush);
      builder.combine(acc, SILO_GPU_OP_AND, operand);
   }
   if (acc == ProgramBuilder::NO_OPERAND) {  // no predicate at all: every row
      acc = builder.allocSlot();
      builder.emit(SILO_GPU_OP_ONES, acc);
   }
   return acc;
}

// ---- BitmapProducer (bitmap_producer.cpp) -----------------------------------------------------------
std::unique_ptr<Operator> BitmapProducer::copy() const {
   return std::make_unique<BitmapProducer>(index, membership, rows);
}
std::unique_ptr<Operator> BitmapProducer::negate() const {
   return std::make_unique<Complement>(this->copy(), rows);
}
uint32_t BitmapProducer::lower(ProgramBuilder& builder) const {
   uint64_t* bitset = builder.temporaryBitset();
   checkGpu(
      silo_gpu_bitset_from_pairs(
         rows.partition->store, bitset, index->device_rows, index->device_ids, static_cast<uint32_t>(index->pair_rows.size()),
         membership.data(), static_cast<uint32_t>(membership.size()), queryStream()
      ),
      "silo_gpu_bitset_from_pairs"
   );
   return SILO_GPU_LEAF_OPERAND + builder.leaf(bitset);
}

// ---- DistanceSelection (no counterpart in the reference) -----------------------------------------------
std::string DistanceSelection::toString() const {
   return "DistanceSelection[<= " + std::to_string(max_distance) + ", compared >= " + std::to_string(min_compared) + "]";
}
std::unique_ptr<Operator> DistanceSelection::copy() const {
   return std::make_unique<DistanceSelection>(seqstore_id, query, max_distance, min_compared, rows);
}
std::unique_ptr<Operator> DistanceSelection::negate() const {
   return std::make_unique<Complement>(this->copy(), rows);
}
uint32_t DistanceSelection::lower(ProgramBuilder& builder) const {
   // 8 bytes per row that never leave the device: the table is written by K11's first entry and read once by the kernel that
   // makes the bitset, all on the query's stream ahead of the fused program; the three buffers live as long as the builder
   const DatabasePartition& partition = *rows.partition;
   const uint32_t row_words = partition.rowWords();
   auto* table = static_cast<uint32_t*>(builder.temporaryBuffer(static_cast<size_t>(row_words) * 64u * 2u * sizeof(uint32_t)));
   void* scratch = builder.temporaryBuffer(SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES(query.size()));
   uint64_t* bitset = builder.temporaryBitset();
   checkGpu(silo_gpu_query_distances(partition.store, seqstore_id, query.data(), table, scratch, queryStream()), "silo_gpu_query_distances");
   checkGpu(
      silo_gpu_bitset_from_distances(table, partition.sequence_count, row_words, max_distance, min_compared, bitset, queryStream()),
      "silo_gpu_bitset_from_distances"
   );
   return SILO_GPU_LEAF_OPERAND + builder.leaf(bitset);
}

// ---- CellCountSelection (no counterpart in the reference) -----------------------------------------------
std::string CellCountSelection::toString() const {
   return "CellCountSelection[" + std::to_string(at_least) + " <= " + filter_expressions::cellKindsString(kinds_mask) + " <= " + std::to_string(at_most) + "]";
}
std::unique_ptr<Operator> CellCountSelection::copy() const {
   return std::make_unique<CellCountSelection>(seqstore_id, kinds_mask, at_least, at_most, rows);
}
std::unique_ptr<Operator> CellCountSelection::negate() const {
   return std::make_unique<Complement>(this->copy(), rows);
}
uint32_t CellCountSelection::lower(ProgramBuilder& builder) const {
   // 16 bytes per row that the store keeps from its first query on (that one computes them and waits); the kernel that makes
   // the bitset reads them once, on the query's stream ahead of the fused program; the bitset lives as long as the builder
   const DatabasePartition& partition = *rows.partition;
   const uint32_t* table = nullptr;
   checkGpu(silo_gpu_store_row_cell_counts(partition.store, seqstore_id, &table, queryStream()), "silo_gpu_store_row_cell_counts");
   uint64_t* bitset = builder.temporaryBitset();
   checkGpu(
      silo_gpu_bitset_from_cell_counts(table, partition.rowWords(), partition.sequence_count, kinds_mask, at_least, at_most, bitset, queryStream()),
      "silo_gpu_bitset_from_cell_counts"
   );
   return SILO_GPU_LEAF_OPERAND + builder.leaf(bitset);
}

// ---- RegionCellCountSelection (no counterpart in the reference) -----------------------------------------
std::string RegionCellCountSelection::toString() const {
   return "RegionCellCountSelection[" + std::to_string(at_least) + " <= " + filter_expressions::cellKindsString(kinds_mask) + " in " +
          std::to_string(first + 1u) + "-" + std::to_string(end) + " <= " + std::to_string(at_most) + "]";
}
std::unique_ptr<Operator> RegionCellCountSelection::copy() const {
   return std::make_unique<RegionCellCountSelection>(seqstore_id, positions, first, end, kinds_mask, at_least, at_most, rows);
}
std::unique_ptr<Operator> RegionCellCountSelection::negate() const {
   return std::make_unique<Complement>(this->copy(), rows);
}
uint32_t RegionCellCountSelection::lower(ProgramBuilder& builder) const {
   // 4 bytes per row that never leave the device: the column is written by K23's first entry and read once by the kernel that
   // makes the bitset, all on the query's stream ahead of the fused program; the three buffers live as long as the builder, and
   // the store keeps nothing of the region
   const DatabasePartition& partition = *rows.partition;
   const uint32_t row_words = partition.rowWords();
   auto* column = static_cast<uint32_t*>(builder.temporaryBuffer(static_cast<size_t>(row_words) * 64u * sizeof(uint32_t)));
   void* scratch = builder.temporaryBuffer(SILO_GPU_REGION_VALUE_SCRATCH_BYTES(positions));
   uint64_t* bitset = builder.temporaryBitset();
   const uint32_t range[2] = {first, end};
   checkGpu(
      silo_gpu_region_cell_values(partition.store, seqstore_id, range, 1, kinds_mask, column, scratch, queryStream()), "silo_gpu_region_cell_values"
   );
   checkGpu(
      silo_gpu_bitset_from_values(column, row_words, partition.sequence_count, at_least, at_most, bitset, queryStream()), "silo_gpu_bitset_from_values"
   );
   return SILO_GPU_LEAF_OPERAND + builder.leaf(bitset);
}

// ---- SampleSelection (no counterpart in the reference) --------------------------------------------------
std::string SampleSelection::toString() const {
   return "SampleSelection[" + std::to_string(size) + " rows" + (range_bounds.empty() ? "" : " of each of " + std::to_string(range_bounds.size() / 2) + " date ranges") +
          ", seed " + std::to_string(seed) + "](" + parts[own].child->toString() + ")";
}
std::unique_ptr<Operator> SampleSelection::copy() const {
   std::vector<Part> copies;
   for (const Part& part : parts) {
      copies.push_back({part.child->copy(), part.dates, part.first_row});
   }
   return std::make_unique<SampleSelection>(std::move(copies), own, size, seed, range_bounds, rows);
}
std::unique_ptr<Operator> SampleSelection::negate() const {
   return std::make_unique<Complement>(this->copy(), rows);
}
uint32_t SampleSelection::lower(ProgramBuilder& builder) const {
   // every partition's rows of the child and, with date ranges, 2 bytes of group per row: they never leave the device.  The
   // thresholds come from one histogram that all partitions add to, so the same request selects the same rows of the database
   // however it is cut into partitions; every launch is on the query's stream, ahead of the fused program.
   struct Evaluated {
      const uint64_t* filter;
      const uint16_t* groups;
      uint32_t sequence_count, row_words, first_row;
   };
   const auto n_ranges = static_cast<uint32_t>(range_bounds.size() / 2);
   void* state = builder.temporaryBuffer(SILO_GPU_SAMPLE_STATE_BYTES(std::max(n_ranges, 1u)));
   std::vector<Evaluated> evaluated;
   for (const Part& part : parts) {
      const DatabasePartition& partition = *part.child->rows.partition;
      OperatorResult result = part.child->evaluate();
      Evaluated rows_of{result.bitset(), nullptr, partition.sequence_count, partition.rowWords(), part.first_row};
      builder.keep(std::move(result));
      if (n_ranges != 0) {
         auto* groups = static_cast<uint16_t*>(builder.temporaryBuffer(static_cast<size_t>(rows_of.row_words) * 64u * sizeof(uint16_t)));
         checkGpu(
            silo_gpu_sample_groups(rows_of.filter, part.dates, range_bounds.data(), n_ranges, rows_of.sequence_count, rows_of.row_words, groups, queryStream()),
            "silo_gpu_sample_groups"
         );
         rows_of.groups = groups;
      }
      evaluated.push_back(rows_of);
   }
   checkGpu(silo_gpu_sample_begin(state, std::max(n_ranges, 1u), size, seed, queryStream()), "silo_gpu_sample_begin");
   for (uint32_t round = 0; round < SILO_GPU_SAMPLE_ROUNDS; ++round) {
      for (const Evaluated& part : evaluated) {
         checkGpu(
            silo_gpu_sample_count(state, part.filter, part.groups, part.sequence_count, part.row_words, part.first_row, round, queryStream()),
            "silo_gpu_sample_count"
         );
      }
      checkGpu(silo_gpu_sample_advance(state, round, queryStream()), "silo_gpu_sample_advance");
   }
   const Evaluated& mine = evaluated[own];
   uint64_t* bitset = builder.temporaryBitset();
   checkGpu(
      silo_gpu_sample_select(state, mine.filter, mine.groups, mine.sequence_count, mine.row_words, mine.first_row, bitset, queryStream()),
      "silo_gpu_sample_select"
   );
   return SILO_GPU_LEAF_OPERAND + builder.leaf(bitset);
}

// ---- DistinctSelection (no counterpart in the reference) ------------------------------------------------
std::string DistinctSelection::toString() const {
   return "DistinctSelection[" + std::to_string(parts.size()) + " partitions](" + parts[own].child->toString() + ")";
}
std::unique_ptr<Operator> DistinctSelection::copy() const {
   std::vector<Part> copies;
   for (const Part& part : parts) {
      copies.push_back({part.child->copy(), part.seqstore_id, part.first_row});
   }
   return std::make_unique<DistinctSelection>(std::move(copies), own, database_rows, rows);
}
std::unique_ptr<Operator> DistinctSelection::negate() const {
   return std::make_unique<Complement>(this->copy(), rows);
}
DistinctTable buildDistinctTable(
   const std::vector<DistinctTable::Part>& parts, uint64_t database_rows, const std::function<const uint64_t*(size_t part)>& rows_of,
   const std::function<void*(size_t bytes)>& allocate, const std::string& what
) {
   DistinctTable built;
   std::vector<silo_gpu_distinct_part> described;
   for (size_t part = 0; part < parts.size(); ++part) {
      const DatabasePartition& partition = *parts[part].partition;
      built.filters.push_back(rows_of(part));
      const uint64_t* hashes = nullptr;
      checkGpu(silo_gpu_store_row_hashes(partition.store, parts[part].seqstore_id, &hashes, queryStream()), "silo_gpu_store_row_hashes");
      described.push_back({hashes, parts[part].first_row, partition.sequence_count, partition.rowWords(), 0});
   }
   uint64_t slots = 2;
   while (slots < 2 * database_rows) {
      slots <<= 1;
   }
   if (slots > (uint64_t{1} << 31)) {
      throw std::runtime_error(what + ": the owner table of a database of more than 2^30 rows exceeds 2^31 slots");
   }
   const size_t parts_bytes = described.size() * sizeof(silo_gpu_distinct_part);
   built.device_parts = static_cast<silo_gpu_distinct_part*>(allocate(parts_bytes));
   built.table = allocate(SILO_GPU_DISTINCT_TABLE_BYTES(slots));
   built.slots = static_cast<uint32_t>(slots);
   built.n_parts = static_cast<uint32_t>(described.size());
   checkGpu(silo_gpu_memcpy_h2d(built.device_parts, described.data(), parts_bytes, queryStream()), "silo_gpu_memcpy_h2d");
   checkGpu(silo_gpu_distinct_begin(built.table, built.slots, queryStream()), "silo_gpu_distinct_begin");
   for (uint32_t part = 0; part < built.n_parts; ++part) {
      checkGpu(
         silo_gpu_distinct_insert(built.table, built.slots, built.device_parts, built.n_parts, part, built.filters[part], queryStream()),
         "silo_gpu_distinct_insert"
      );
   }
   return built;
}

uint32_t DistinctSelection::lower(ProgramBuilder& builder) const {
   // every partition's rows of the child and its store's kept row hashes (the first query on a store computes them and waits: that
   // request pays for the build) never leave the device.  One owner table takes the rows of all partitions, so a class is
   // represented by its smallest row number in the database however the database is cut; every launch is on the query's stream,
   // ahead of the fused program.
   std::vector<DistinctTable::Part> described;
   for (const Part& part : parts) {
      described.push_back({part.child->rows.partition, part.seqstore_id, part.first_row});
   }
   const DistinctTable built = buildDistinctTable(
      described, database_rows,
      [&](size_t part) {
         OperatorResult result = parts[part].child->evaluate();
         const uint64_t* filter = result.bitset();
         builder.keep(std::move(result));
         return filter;
      },
      [&](size_t bytes) { return builder.temporaryBuffer(bytes); }, "DistinctSequences"
   );
   uint64_t* bitset = builder.temporaryBitset();
   checkGpu(
      silo_gpu_distinct_select(built.table, built.slots, built.device_parts, built.n_parts, own, built.filters[own], bitset, queryStream()),
      "silo_gpu_distinct_select"
   );
   return SILO_GPU_LEAF_OPERAND + builder.leaf(bitset);
}

// ---- BitmapSelection (bitmap_selection.cpp:33-71) -----------------------------------------------
std::unique_ptr<Operator> BitmapSelection::copy() const {
   auto out = std::make_unique<BitmapSelection>(*this);
   return out;
}
std::unique_ptr<Operator> BitmapSelection::negate() const {
   auto out = std::make_unique<BitmapSelection>(*this);
   out->comparator = comparator == CONTAINS ? NOT_CONTAINS : CONTAINS;
   return out;
}
const uint64_t* BitmapSelection::storedColumn(ProgramBuilder& builder) const {
   if (comparator != CONTAINS) {
      return nullptr;
   }
   return materialise ? builder.sparsePointer(seqstore_id, local_position, symbol) : missing_plane;
}
uint32_t BitmapSelection::lower(ProgramBuilder& builder) const {
   const uint32_t operand = SILO_GPU_LEAF_OPERAND + (materialise ? builder.sparseLeaf(seqstore_id, local_position, symbol) : builder.leaf(missing_plane));
   if (comparator == CONTAINS) {
      return operand;
   }
   const uint32_t slot = builder.allocSlot();
   builder.emit(SILO_GPU_OP_NOT, slot, operand);
   return slot;
}

// ---- Complement (complement.cpp) ----------------------------------------------------------------
std::unique_ptr<Operator> Complement::copy() const {
   return std::make_unique<Complement>(child->copy(), rows);
}
std::unique_ptr<Operator> Complement::negate() const {
   return child->copy();
}
uint32_t Complement::lower(ProgramBuilder& builder) const {  // flip(0,row_count): complement.cpp:50-54
   const uint32_t operand = builder.lowerChild(*child);
   const uint32_t slot = isLeafOperand(operand) ? builder.allocSlot() : operand;
   builder.emit(SILO_GPU_OP_NOT, slot, operand);
   return slot;
}
Cost Complement::cost() const {
   Cost c = child->cost();
   c.instructions += 1;
   c.slots = std::max(c.slots, 1u);
   return c;
}

// ---- Intersection (intersection.cpp) ------------------------------------------------------------
Intersection::Intersection(OperatorVector&& children_, OperatorVector&& negated_children_, RowSpace rows)
    : Operator(rows), children(std::move(children_)), negated_children(std::move(negated_children_)) {
   if (children.empty()) {
      throw QueryCompilationException(
         "Compilation bug: Intersection without non-negated children is not allowed. Should be compiled as a union."
      );
   }
   if (children.size() + negated_children.size() < 2) {
      throw QueryCompilationException("Compilation bug: Intersection needs at least two children.");
   }
}
std::string Intersection::toString() const {
   std::string res = "(" + children[0]->toString();
   for (size_t i = 1; i < children.size(); ++i) {
      res += " & " + children[i]->toString();
   }
   for (const auto& child : negated_children) {
      res += " &! " + child->toString();
   }
   return res + ")";
}
std::unique_ptr<Operator> Intersection::copy() const {
   return std::make_unique<Intersection>(copyAll(children), copyAll(negated_children), rows);
}
std::unique_ptr<Operator> Intersection::negate() const {
   return std::make_unique<Complement>(copy(), rows);
}
uint32_t Intersection::lower(ProgramBuilder& builder) const {
   // The reference orders children by cardinality to keep roaring intermediates small
   // (intersection.cpp:94-108); a dense word-parallel AND has no such sensitivity.  Children that are
   // stored columns are folded by ONE n-ary instruction (streamed 8 loads at a time).
   // A node too wide for one program (only the root of a program is) is folded in pieces: see ProgramBuilder::flush.
   const bool may_flush = builder.empty();
   const ProgramBuilder::Split positive = builder.split(children);
   const ProgramBuilder::Split negative = builder.split(negated_children);
   uint32_t acc = ProgramBuilder::NO_OPERAND;
   builder.foldColumns(acc, SILO_GPU_OP_AND_N, SILO_GPU_OP_AND, positive.columns, may_flush);
   for (const Operator* child : positive.composite) {
      const uint32_t operand = builder.lowerChildBeside(acc, *child, may_flush);
      builder.combine(acc, SILO_GPU_OP_AND, operand);
   }
   // children is never empty (constructor), so acc is set here; acc &~ (a | b) = (acc &~ a) &~ b lets the negated runs be cut too
   builder.foldColumns(acc, SILO_GPU_OP_OR_N, SILO_GPU_OP_ANDNOT, negative.columns, may_flush);
   for (const Operator* child : negative.composite) {
      const uint32_t operand = builder.lowerChildBeside(acc, *child, may_flush);
      builder.combine(acc, SILO_GPU_OP_ANDNOT, operand);
   }
   return acc;
}
Cost Intersection::cost() const {
   return sumCost(children, &negated_children).total;
}

// ---- Union (union.cpp) --------------------------------------------------------------------------
std::string Union::toString() const {
   if (children.empty()) {
      return "()";
   }
   std::string res = "(" + children[0]->toString();
   for (size_t i = 1; i < children.size(); ++i) {
      res += " | " + children[i]->toString();
   }
   return res + ")";
}
std::unique_ptr<Operator> Union::copy() const {
   return std::make_unique<Union>(copyAll(children), rows);
}
std::unique_ptr<Operator> Union::negate() const {
   return std::make_unique<Complement>(copy(), rows);
}
uint32_t Union::lower(ProgramBuilder& builder) const {
   if (children.empty()) {  // union.test.cpp:28-34: the union of nothing is empty
      const uint32_t slot = builder.allocSlot();
      builder.emit(SILO_GPU_OP_ZERO, slot);
      return slot;
   }
   const bool may_flush = builder.empty();
   const ProgramBuilder::Split parts = builder.split(children);
   uint32_t acc = ProgramBuilder::NO_OPERAND;
   // roaring fastunion (union.cpp:44) -> one streamed n-ary OR (several, with a flush between them, beyond the leaves of a program)
   builder.foldColumns(acc, SILO_GPU_OP_OR_N, SILO_GPU_OP_OR, parts.columns, may_flush);
   for (const Operator* child : parts.composite) {
      const uint32_t operand = builder.lowerChildBeside(acc, *child, may_flush);
      builder.combine(acc, SILO_GPU_OP_OR, operand);
   }
   return acc;
}
Cost Union::cost() const {
   Cost c = sumCost(children).total;
   c.instructions += 1;
   return c;
}

// ---- Threshold (threshold.cpp) ------------------------------------------------------------------
Threshold::Threshold(OperatorVector&& non_negated_children_, OperatorVector&& negated_children_, uint32_t number_of_matchers, bool match_exactly, RowSpace rows)
    : Operator(rows),
      non_negated_children(std::move(non_negated_children_)),
      negated_children(std::move(negated_children_)),
      number_of_matchers(number_of_matchers),
      match_exactly(match_exactly) {
   if (number_of_matchers >= non_negated_children.size() + negated_children.size()) {  // threshold.cpp:28-33
      throw QueryCompilationException(
         "Compilation Error: number_of_matchers must be less than the number of children of a threshold expression"
      );
   }
   if (number_of_matchers == 0) {
      throw QueryCompilationException("Compilation Error: number_of_matchers must be greater than zero");
   }
}
std::string Threshold::toString() const {
   std::string res = match_exactly ? "=" : ">=";
   for (const auto& child : non_negated_children) {
      res += ", " + child->toString();
   }
   for (const auto& child : negated_children) {
      res += ", ! " + child->toString();
   }
   return res + ")";
}
std::unique_ptr<Operator> Threshold::copy() const {
   return std::make_unique<Threshold>(copyAll(non_negated_children), copyAll(negated_children), number_of_matchers, match_exactly, rows);
}
std::unique_ptr<Operator> Threshold::negate() const {
   return std::make_unique<Complement>(copy(), rows);
}
uint32_t Threshold::lower(ProgramBuilder& builder) const {
   // The reference keeps a DP table of n (or n+1) bitmaps, table[j] = rows matched by > j children
   // so far (threshold.cpp:64-138).  Word-parallel restatement: a bit-sliced per-row counter of
   // ceil(log2(k+1)) slots, one ripple-carry add per child, one comparison with n at the end.
   const uint32_t k = static_cast<uint32_t>(non_negated_children.size() + negated_children.size());
   const uint32_t bits = static_cast<uint32_t>(std::bit_width(k));
   const ProgramBuilder::Split positive = builder.split(non_negated_children);
   const ProgramBuilder::Split negative = builder.split(negated_children);
   if (builder.empty() && !builder.fits(cost())) {  // the root of a program, and possibly too wide for one
      return lowerInPieces(builder, positive, negative, bits);
   }
   const uint32_t counter = builder.allocRun(bits);
   for (uint32_t bit = 0; bit < bits; ++bit) {
      builder.emit(SILO_GPU_OP_ZERO, counter + bit);
   }
   if (!positive.columns.empty()) {
      builder.emit(SILO_GPU_OP_CNT_ADD_N, counter, 0, bits, builder.leafRun(positive.columns));
   }
   if (!negative.columns.empty()) {
      builder.emit(SILO_GPU_OP_CNT_ADD_NOT_N, counter, 0, bits, builder.leafRun(negative.columns));
   }
   for (const Operator* child : positive.composite) {
      const uint32_t tmp = builder.lowerChild(*child);
      builder.emit(SILO_GPU_OP_CNT_ADD, counter, tmp, bits);
      builder.freeSlot(tmp);
   }
   for (const Operator* child : negative.composite) {
      const uint32_t operand = builder.lowerChild(*child);
      const uint32_t tmp = isLeafOperand(operand) ? builder.allocSlot() : operand;
      builder.emit(SILO_GPU_OP_NOT, tmp, operand);
      builder.emit(SILO_GPU_OP_CNT_ADD, counter, tmp, bits);
      builder.freeSlot(tmp);
   }
   const uint32_t result = builder.allocSlot();
   builder.emit(match_exactly ? SILO_GPU_OP_CNT_EQ : SILO_GPU_OP_CNT_GE, result, counter, bits, number_of_matchers);
   builder.freeRun(counter, bits);
   return result;
}

uint32_t Threshold::lowerInPieces(
   ProgramBuilder& builder, const ProgramBuilder::Split& positive, const ProgramBuilder::Split& negative, uint32_t bits
) const {
   // The counter lives in slots and a program hands out one slot.  So a program that is full is run once per plane of its partial
   // count (ProgramBuilder::flushPlanes), and plane j comes back as a term of weight 1 << j, which CNT_ADD adds into the next
   // program's counter from bit j up.  The terms are taken in the order of lower(), planes last: a node that does fit one
   // program gets the program of lower().  Every program takes more terms than the planes it returns, so this ends.  A composite
   // child that fits no program is evaluated on its own by lowerChild; when terms were taken before it, the program is cut in
   // front of it first (it might have fitted the next one), which costs a round of plane launches per such child.
   struct Term {
      const uint64_t* column;     // a stored column, or a plane of a partial count
      const Operator* composite;  // or a sub-tree
      bool negated;
      uint32_t shift;
   };
   std::deque<Term> terms;
   for (const uint64_t* column : positive.columns) {
      terms.push_back({column, nullptr, false, 0});
   }
   for (const uint64_t* column : negative.columns) {
      terms.push_back({column, nullptr, true, 0});
   }
   for (const Operator* child : positive.composite) {
      terms.push_back({nullptr, child, false, 0});
   }
   for (const Operator* child : negative.composite) {
      terms.push_back({nullptr, child, true, 0});
   }
   const size_t first_plane = terms.size();  // the terms before it are the children
   size_t taken = 0;
   while (true) {
      const uint32_t counter = builder.allocRun(bits);
      for (uint32_t bit = 0; bit < bits; ++bit) {
         builder.emit(SILO_GPU_OP_ZERO, counter + bit);
      }
      uint64_t largest = 0;  // the largest count this program can reach
      bool full = false;
      while (taken < terms.size() && !full) {
         const Term term = terms[taken];
         if (term.composite != nullptr) {
            const Cost cost = term.composite->cost();
            if (largest > 0 && !builder.fits(cost)) {
               full = true;
               continue;
            }
            uint32_t operand = builder.lowerChild(*term.composite, cost);
            if (term.negated) {
               const uint32_t tmp = isLeafOperand(operand) ? builder.allocSlot() : operand;
               builder.emit(SILO_GPU_OP_NOT, tmp, operand);
               operand = tmp;
            }
            builder.emit(SILO_GPU_OP_CNT_ADD, counter, operand, bits);
            builder.freeSlot(operand);
            largest += 1;
            ++taken;
         } else if (!builder.hasRoom(1, 2)) {
            full = true;
         } else if (taken >= first_plane) {
            builder.emit(SILO_GPU_OP_CNT_ADD, counter + term.shift, SILO_GPU_LEAF_OPERAND + builder.leaf(term.column), bits - term.shift);
            largest += uint64_t{1} << term.shift;
            ++taken;
         } else {  // the run of columns of this sign, or as much of it as fits
            std::vector<const uint64_t*> columns;
            while (taken < first_plane && columns.size() < builder.leafRoom() && terms[taken].composite == nullptr && terms[taken].negated == term.negated) {
               columns.push_back(terms[taken++].column);
            }
            builder.emit(term.negated ? SILO_GPU_OP_CNT_ADD_NOT_N : SILO_GPU_OP_CNT_ADD_N, counter, 0, bits, builder.leafRun(columns));
            largest += columns.size();
         }
      }
      if (taken == terms.size()) {
         const uint32_t result = builder.allocSlot();
         builder.emit(match_exactly ? SILO_GPU_OP_CNT_EQ : SILO_GPU_OP_CNT_GE, result, counter, bits, number_of_matchers);
         builder.freeRun(counter, bits);
         return result;
      }
      // no count exceeds k < 1 << bits, so `bits` planes hold any partial count
      const uint32_t planes = std::min(bits, static_cast<uint32_t>(std::bit_width(largest)));
      const std::vector<const uint64_t*> partial = builder.flushPlanes(counter, planes);
      for (uint32_t plane = 0; plane < planes; ++plane) {
         terms.push_back({partial[plane], nullptr, false, plane});
      }
   }
}
Cost Threshold::cost() const {
   // what lower() emits: the ZEROs of the counter, an n-ary add per sign, the comparison; the counter beside the widest child
   const uint32_t bits = static_cast<uint32_t>(std::bit_width(non_negated_children.size() + negated_children.size()));
   const FoldCost children = sumCost(non_negated_children, &negated_children);
   Cost c = children.total;
   c.instructions += bits + 3;
   c.slots = bits + std::max(children.widest_child, 1u);
   return c;
}

}  // namespace operators
}  // namespace silo::query_engine
