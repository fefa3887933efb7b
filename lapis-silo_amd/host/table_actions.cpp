// table_actions.cpp — the actions that answer from one small table of counts filled on the device: MutationsOverTime<SymbolType>
// (K7), QueriesOverTime (K8) and CrossTabulation (K9), which fetch the table, and Consensus<SymbolType> (K15),
// MutationsComparison<SymbolType> (K17) and MeanDistances<SymbolType> (K24), which fetch what a last kernel makes of the tables of their
// groups, with their parsers (that of MeanDistances: actions.cpp).
// Each differs in the kernel call of a partition and in the rows it makes of the table; what stands around that — the refusals, the
// date column, the table's life on the device, the evaluation of labelled sub-expressions, the tables of named groups and what has
// to stay alive while launches run — is here once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <set>
#include <string_view>

#include "query_engine.h"

namespace silo::query_engine::actions {

// ---- what the three actions share (requireUnsharded and the two stream guards: with every action that launches on its own) ----
void requireUnsharded(const Database& database, const std::string& action_name) {
   CHECK_SILO_QUERY(
      database.shard_world <= 1, action_name + " is not supported on a sharded database yet: its counts are not all-reduced across ranks"
   )
}

void waitIfThrown(const std::function<void()>& launches) {
   try {
      launches();
   } catch (...) {
      // launches of this query may be in flight on the stream: let them finish before its buffers return to the pool
      (void)silo_gpu_stream_synchronize(queryStream());
      throw;
   }
}

void launchAndWait(const std::function<void()>& launches) {
   waitIfThrown([&] {
      launches();
      // a copy was the last thing enqueued, but say it: nothing of this query runs any more when its buffers go back
      checkGpu(silo_gpu_stream_synchronize(queryStream()), "silo_gpu_stream_synchronize");
   });
}

namespace {

std::string notADateColumn(const std::string& date_field, const std::string& action_name) {
   return "The field dateField of " + action_name + " ('" + date_field + "') is not a date column";
}

/// The configuration knows `date_field` as a date column.
void requireDateColumn(const Database& database, const std::string& date_field, const std::string& action_name) {
   const std::optional<storage::ColumnMetadata> column = database.database_config.getMetadata(date_field);
   CHECK_SILO_QUERY(column.has_value() && column->type == config::ColumnType::DATE, notADateColumn(date_field, action_name))
}

/// The dates of a partition's rows on the device, one uint32 per row.
const uint32_t* deviceDates(const DatabasePartition& partition, const std::string& date_field, const std::string& action_name) {
   const auto* dates = partition.columns.find(date_field, config::ColumnType::DATE);
   CHECK_SILO_QUERY(dates != nullptr, notADateColumn(date_field, action_name))
   return static_cast<const uint32_t*>(dates->deviceValues());
}

/// (from, to) per range as K7 / K8 take them: both inclusive, an open end as the least / greatest date (0 is the NULL date).
std::vector<uint32_t> dateBounds(const std::vector<OverTimeDateRange>& date_ranges) {
   std::vector<uint32_t> bounds;
   bounds.reserve(2 * date_ranges.size());
   for (const OverTimeDateRange& range : date_ranges) {
      bounds.push_back(range.from.value_or(common::Date{1}));
      bounds.push_back(range.to.value_or(common::Date{UINT32_MAX}));
   }
   return bounds;
}

/// An end of a range in a result row: null when open.
JsonValue dateText(const std::optional<common::Date>& date) {
   if (!date.has_value()) {
      return std::nullopt;
   }
   return common::dateToString(*date).value_or("");
}

/// What launches on queryStream() read besides the table: the bitsets of sub-expressions (kept per side: CrossTabulation has
/// two) and scratch.  Nothing in it returns to the pool while a launch that was given it may still run: bitsets leave only
/// through waitAndRelease, a scratch only once the stream has been waited for after it was handed out.
class LiveSet {
   std::vector<OperatorResult> filters[2];
   std::vector<DeviceBuffer> scratches;
   bool in_flight = false;  // scratch was handed out since the last wait: launches may be running

  public:
   /// Scratch for the launches that follow.  Those handed out before stay unless the stream was waited for since.
   void* scratch(const DatabasePartition& partition, size_t bytes) {
      DeviceBuffer fresh = partition.pool.acquire(bytes);
      if (!in_flight) {
         scratches.clear();
      }
      scratches.push_back(std::move(fresh));
      in_flight = true;
      return scratches.back().get();
   }
   /// Launches that read kept bitsets, but took no scratch, were enqueued: waitAndRelease has something to wait for.
   void launched() { in_flight = true; }
   /// Keeps the bitset of a sub-expression for the launches that follow.
   const uint64_t* keep(OperatorResult result, size_t side = 0) {
      const uint64_t* bits = result.bitset();
      filters[side].push_back(std::move(result));
      return bits;
   }
   /// Launches since the last wait may still read the bitsets: wait for them, then those of `side` return to the pool.
   void waitAndRelease(size_t side = 0) {
      if (in_flight) {
         checkGpu(silo_gpu_stream_synchronize(queryStream()), "silo_gpu_stream_synchronize");
         in_flight = false;
      }
      filters[side].clear();
   }
};

/// The launches of one partition into the table.  base_bits: the rows of the query's filter, nullptr when it selects every row.
using PartitionLaunches = std::function<void(const DatabasePartition& partition, const uint64_t* base_bits, uint32_t* device_table, LiveSet& live)>;

/// The life of a table of `words` uint32 counts: zeroed on the device (pool of the first partition), filled by `launches` for
/// every partition whose filter selects a row, fetched once.  Empty for a database without partitions.  If anything throws,
/// the stream is waited for before the table and the live set return to the pool.
std::vector<uint32_t> countTable(
   const Database& database, const std::vector<OperatorResult>& bitmap_filter, size_t words, const PartitionLaunches& launches
) {
   std::vector<uint32_t> table;
   if (database.partitions.empty()) {
      return table;
   }
   DeviceBuffer device_table = database.partitions.front().pool.acquire(words * sizeof(uint32_t));
   checkGpu(silo_gpu_memset_async(device_table.get(), 0, words * sizeof(uint32_t), queryStream()), "silo_gpu_memset_async");
   LiveSet live;  // kept until the table has landed: the launches read it
   HostFetch fetch;
   waitIfThrown([&] {
      for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
         const DatabasePartition& partition = database.partitions[partition_id];
         const OperatorResult& filter = bitmap_filter[partition_id];
         const uint32_t selected = partition.sequence_count == 0 ? 0 : filter.cardinality();
         if (selected == 0) {
            continue;
         }
         // a filter that selects every row is passed as NULL (no all-ones bitset is made for it)
         launches(partition, selected == partition.sequence_count ? nullptr : filter.bitset(), device_table.as<uint32_t>(), live);
      }
      fetch = HostFetch(device_table.get(), words * sizeof(uint32_t), queryStream());
      const auto* host = static_cast<const uint32_t*>(fetch.wait());
      table.assign(host, host + words);
   });
   return table;
}

/// A labelled sub-expression on one partition: the rows it selects and, unless those are none or all, their bitset.
struct SubFilter {
   uint32_t cardinality;
   OperatorResult result;
};

/// Compiled and evaluated as the top-level filter is (compileFilter, query_engine.cpp).
SubFilter evaluateSubFilter(const Database& database, const DatabasePartition& partition, const filter_expressions::Expression& expression) {
   std::unique_ptr<operators::Operator> root = expression.compile(database, partition, filter_expressions::Expression::AmbiguityMode::NONE);
   const operators::Type type = root->type();
   SubFilter sub{type == operators::FULL ? partition.sequence_count : 0, {}};
   if (type != operators::EMPTY && type != operators::FULL) {
      sub.result = operators::Operator::evaluate(std::move(root));
      sub.result.materialize();  // one launch yields both the bitset and its cardinality
      sub.cardinality = sub.result.cardinality();
   }
   return sub;
}

}  // namespace

// ---- MutationsOverTime ---------------------------------------------------------------------------------
template <typename SymbolType>
void MutationsOverTime<SymbolType>::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"mutation", "sequenceName", "dateFrom", "dateTo", "count", "coverage"});
}

template <typename SymbolType>
QueryResult MutationsOverTime<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = std::is_same_v<SymbolType, Nucleotide> ? "MutationsOverTime" : "AminoAcidMutationsOverTime";
   requireUnsharded(database, action_name);
   requireDateColumn(database, date_field, action_name);

   // resolve every mutation against its sequence store: the name, the 0-based position, the reference symbol
   struct Resolved {
      std::string sequence_name;
      const SequenceStore<SymbolType>* store;
      uint32_t position;  // 0-based
   };
   std::vector<Resolved> resolved;
   resolved.reserve(mutations.size());
   for (const Mutation& mutation : mutations) {
      const auto [name, store] = sequenceStoreOf<SymbolType>(
         database, mutation.sequence_name, "Database does not contain the " + std::string(SymbolType::SYMBOL_NAME_LOWER_CASE) + " sequence with name: "
      );
      const auto& reference = store.reference_sequence;
      CHECK_SILO_QUERY(
         mutation.position >= 1 && mutation.position <= reference.size(),
         "The position " + std::to_string(mutation.position) + " of a mutation of " + action_name + " is outside the sequence '" + name + "' (1 to " +
            std::to_string(reference.size()) + ")"
      )
      const auto reference_symbol = reference[mutation.position - 1];
      if (mutation.reference_symbol.has_value()) {
         CHECK_SILO_QUERY(
            SymbolType::charToSymbol(*mutation.reference_symbol) == reference_symbol,
            std::string("The reference symbol '") + *mutation.reference_symbol + "' of a mutation of " + action_name + " does not match the reference genome ('" +
               SymbolType::symbolToChar(reference_symbol) + "' at position " + std::to_string(mutation.position) + " of '" + name + "')"
         )
      }
      resolved.push_back({name, &store, mutation.position - 1});
   }

   // the table: one block of rows per sequence store touched, the store's mutations in request order within it
   const auto n_ranges = static_cast<uint32_t>(date_ranges.size());
   std::vector<std::string> store_names;
   std::vector<std::vector<uint32_t>> members;  // request indices per store
   for (uint32_t m = 0; m < resolved.size(); ++m) {
      const auto s = static_cast<size_t>(std::find(store_names.begin(), store_names.end(), resolved[m].sequence_name) - store_names.begin());
      if (s == store_names.size()) {
         store_names.push_back(resolved[m].sequence_name);
         members.emplace_back();
      }
      members[s].push_back(m);
   }
   std::vector<uint32_t> row_of(resolved.size());  // request index -> row of the table
   std::vector<uint32_t> first_row(store_names.size());
   uint32_t rows = 0;
   for (size_t s = 0; s < store_names.size(); ++s) {
      first_row[s] = rows;
      for (const uint32_t m : members[s]) {
         row_of[m] = rows++;
      }
   }
   const std::vector<uint32_t> bounds = dateBounds(date_ranges);

   std::vector<uint32_t> table;
   const size_t table_words = static_cast<size_t>(rows) * n_ranges * 2u;
   if (table_words != 0) {
      table = countTable(
         database, bitmap_filter, table_words,
         [&](const DatabasePartition& partition, const uint64_t* base_bits, uint32_t* device_table, LiveSet& live) {
            const uint32_t* dates = deviceDates(partition, date_field, action_name);
            for (size_t s = 0; s < store_names.size(); ++s) {  // one K7 call per store; every scratch stays until the table has landed
               const SequenceStorePartition<SymbolType>& store = partition.getSequenceStores<SymbolType>().at(store_names[s]);
               std::vector<uint32_t> positions, symbols;
               for (const uint32_t m : members[s]) {
                  positions.push_back(resolved[m].position);
                  symbols.push_back(static_cast<uint32_t>(mutations[m].symbol));
               }
               const auto n = static_cast<uint32_t>(positions.size());
               void* scratch = live.scratch(partition, SILO_GPU_GROUPED_SCRATCH_BYTES(partition.rowWords(), n_ranges, n));
               checkGpu(
                  silo_gpu_mutations_grouped(
                     store.store, store.seqstore_id, base_bits, dates, bounds.data(), n_ranges, positions.data(), symbols.data(), n, scratch,
                     device_table + static_cast<size_t>(first_row[s]) * n_ranges * 2u, queryStream()
                  ),
                  "silo_gpu_mutations_grouped"
               );
            }
         }
      );
   }

   std::vector<QueryResultEntry> result_rows;
   result_rows.reserve(resolved.size() * n_ranges);
   for (size_t m = 0; m < resolved.size(); ++m) {
      const char from = SymbolType::symbolToChar(resolved[m].store->reference_sequence.at(resolved[m].position));
      const std::string name = from + std::to_string(resolved[m].position + 1) + SymbolType::symbolToChar(mutations[m].symbol);
      for (uint32_t r = 0; r < n_ranges; ++r) {
         const size_t cell = (static_cast<size_t>(row_of[m]) * n_ranges + r) * 2u;
         const uint32_t count = table.empty() ? 0u : table[cell];
         const uint32_t coverage = table.empty() ? 0u : table[cell + 1u];
         QueryResultEntry& entry = result_rows.emplace_back();
         entry.fields.emplace("count", static_cast<int32_t>(count));
         entry.fields.emplace("coverage", static_cast<int32_t>(coverage));
         entry.fields.emplace("dateFrom", dateText(date_ranges[r].from));
         entry.fields.emplace("dateTo", dateText(date_ranges[r].to));
         entry.fields.emplace("mutation", name);
         entry.fields.emplace("sequenceName", resolved[m].sequence_name);
      }
   }
   return QueryResult{std::move(result_rows)};
}

template class MutationsOverTime<Nucleotide>;
template class MutationsOverTime<AminoAcid>;

// ---- QueriesOverTime -----------------------------------------------------------------------------------
void QueriesOverTime::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"displayLabel", "dateFrom", "dateTo", "count", "coverage"});
}

QueryResult QueriesOverTime::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = "QueriesOverTime";
   requireUnsharded(database, action_name);
   requireDateColumn(database, date_field, action_name);
   const auto n_ranges = static_cast<uint32_t>(date_ranges.size());
   const auto n_filters = static_cast<uint32_t>(filters.size());
   const std::vector<uint32_t> bounds = dateBounds(date_ranges);

   // one table [distinct sub-expression][range], accumulated over the partitions
   std::vector<uint32_t> table;
   const size_t table_words = static_cast<size_t>(n_filters) * n_ranges;
   if (table_words != 0) {
      table = countTable(
         database, bitmap_filter, table_words,
         [&](const DatabasePartition& partition, const uint64_t* base_bits, uint32_t* device_table, LiveSet& live) {
            const uint32_t* dates = deviceDates(partition, date_field, action_name);
            for (uint32_t batch_begin = 0; batch_begin < n_filters; batch_begin += MAX_LIVE_FILTERS) {
               const uint32_t batch_end = std::min(n_filters, batch_begin + MAX_LIVE_FILTERS);
               live.waitAndRelease();  // the launches of the batch before may still read its bitsets
               void* scratch = live.scratch(partition, SILO_GPU_FILTERS_GROUPED_SCRATCH_BYTES(partition.rowWords(), n_ranges, batch_end - batch_begin));
               // K8 counts filters that stand side by side in the table: a sub-expression that selects no row here ends a run
               uint32_t run_begin = batch_begin;
               std::vector<const uint64_t*> run;
               const auto launchRun = [&]() {
                  if (!run.empty()) {
                     checkGpu(
                        silo_gpu_filters_grouped(
                           partition.store, base_bits, dates, bounds.data(), n_ranges, run.data(), static_cast<uint32_t>(run.size()), scratch,
                           device_table + static_cast<size_t>(run_begin) * n_ranges, queryStream()
                        ),
                        "silo_gpu_filters_grouped"
                     );
                     run.clear();
                  }
               };
               for (uint32_t f = batch_begin; f < batch_end; ++f) {
                  SubFilter sub = evaluateSubFilter(database, partition, *filters[f]);
                  if (sub.cardinality == 0) {  // its cells stay 0
                     launchRun();
                     run_begin = f + 1;
                     continue;
                  }
                  // all rows: no bitset is read
                  run.push_back(sub.cardinality == partition.sequence_count ? nullptr : live.keep(std::move(sub.result)));
               }
               launchRun();
            }
         }
      );
   }

   std::vector<QueryResultEntry> result_rows;
   result_rows.reserve(queries.size() * n_ranges);
   for (const LabelledQuery& query : queries) {
      for (uint32_t r = 0; r < n_ranges; ++r) {
         const uint32_t count = table.empty() ? 0u : table[static_cast<size_t>(query.count_filter) * n_ranges + r];
         const uint32_t coverage = table.empty() ? 0u : table[static_cast<size_t>(query.coverage_filter) * n_ranges + r];
         QueryResultEntry& entry = result_rows.emplace_back();
         entry.fields.emplace("count", static_cast<int32_t>(count));
         entry.fields.emplace("coverage", static_cast<int32_t>(coverage));
         entry.fields.emplace("dateFrom", dateText(date_ranges[r].from));
         entry.fields.emplace("dateTo", dateText(date_ranges[r].to));
         entry.fields.emplace("displayLabel", query.display_label);
      }
   }
   return QueryResult{std::move(result_rows)};
}

// ---- CrossTabulation -----------------------------------------------------------------------------------
void CrossTabulation::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"rowLabel", "columnLabel", "count", "rowCount", "columnCount", "total"});
}

QueryResult CrossTabulation::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   requireUnsharded(database, "CrossTabulation");
   // one table [distinct row sub-expression + 1][distinct column sub-expression + 1], accumulated over the partitions: the last
   // row and the last column belong to an all-rows entry, so the marginals and the total come out of the same pass
   const auto n_row_filters = static_cast<uint32_t>(row_filters.size());
   const auto n_column_filters = static_cast<uint32_t>(column_filters.size());
   const uint32_t table_rows = n_row_filters + 1u;
   const uint32_t table_columns = n_column_filters + 1u;
   std::vector<uint32_t> table;
   if (!row_queries.empty() && !column_queries.empty()) {
      constexpr uint32_t SIDE_BATCH = MAX_LIVE_FILTERS / 2;
      enum Side : size_t { ROWS, COLUMNS };
      table = countTable(
         database, bitmap_filter, static_cast<size_t>(table_rows) * table_columns,
         [&](const DatabasePartition& partition, const uint64_t* base_bits, uint32_t* device_table, LiveSet& live) {
            // entries [begin, end) of one side (the entry past the side's last sub-expression is all rows): the bitsets and where
            // each lands in the table; a sub-expression that selects no row here is left out, one that selects every row is NULL
            const auto evaluateSide = [&](Side which, uint32_t begin, uint32_t end, std::vector<const uint64_t*>& bitsets, std::vector<uint32_t>& index) {
               const std::vector<uint32_t>& side = which == ROWS ? row_filters : column_filters;
               bitsets.clear();
               index.clear();
               for (uint32_t entry = begin; entry < end; ++entry) {
                  if (entry == side.size()) {
                     bitsets.push_back(nullptr);
                     index.push_back(entry);
                     continue;
                  }
                  SubFilter sub = evaluateSubFilter(database, partition, *filters[side[entry]]);
                  if (sub.cardinality == 0) {  // its cells stay 0
                     continue;
                  }
                  index.push_back(entry);
                  // all rows: no bitset is read
                  bitsets.push_back(sub.cardinality == partition.sequence_count ? nullptr : live.keep(std::move(sub.result), which));
               }
            };
            std::vector<const uint64_t*> row_bitsets, column_bitsets;
            std::vector<uint32_t> row_index, column_index;
            for (uint32_t row_begin = 0; row_begin < table_rows; row_begin += SIDE_BATCH) {
               live.waitAndRelease(ROWS);  // a launch may still read the bitsets of the batch before
               evaluateSide(ROWS, row_begin, std::min(table_rows, row_begin + SIDE_BATCH), row_bitsets, row_index);
               if (row_bitsets.empty()) {
                  continue;
               }
               // the column side is streamed past every row batch: a column sub-expression is evaluated once per row batch
               for (uint32_t column_begin = 0; column_begin < table_columns; column_begin += SIDE_BATCH) {
                  live.waitAndRelease(COLUMNS);
                  evaluateSide(COLUMNS, column_begin, std::min(table_columns, column_begin + SIDE_BATCH), column_bitsets, column_index);
                  if (column_bitsets.empty()) {
                     continue;
                  }
                  const auto n_rows = static_cast<uint32_t>(row_bitsets.size());
                  const auto n_columns = static_cast<uint32_t>(column_bitsets.size());
                  void* scratch = live.scratch(partition, SILO_GPU_FILTERS_CROSS_SCRATCH_BYTES(n_rows, n_columns));
                  checkGpu(
                     silo_gpu_filters_cross(
                        partition.store, base_bits, row_bitsets.data(), row_index.data(), n_rows, column_bitsets.data(), column_index.data(), n_columns,
                        scratch, device_table, table_rows, table_columns, queryStream()
                     ),
                     "silo_gpu_filters_cross"
                  );
               }
            }
         }
      );
   }

   const auto cell = [&](uint32_t row, uint32_t column) {
      return table.empty() ? int32_t{0} : static_cast<int32_t>(table[static_cast<size_t>(row) * table_columns + column]);
   };
   std::vector<QueryResultEntry> result_rows;
   result_rows.reserve(row_queries.size() * column_queries.size());
   for (const LabelledQuery& row : row_queries) {
      for (const LabelledQuery& column : column_queries) {
         QueryResultEntry& entry = result_rows.emplace_back();
         entry.fields.emplace("rowLabel", row.display_label);
         entry.fields.emplace("columnLabel", column.display_label);
         entry.fields.emplace("count", cell(row.slot, column.slot));
         entry.fields.emplace("rowCount", cell(row.slot, n_column_filters));
         entry.fields.emplace("columnCount", cell(n_row_filters, column.slot));
         entry.fields.emplace("total", cell(n_row_filters, n_column_filters));
      }
   }
   return QueryResult{std::move(result_rows)};
}

// ---- Consensus -------------------------------------------------------------------------------------------
// The consensus sequence of the query's filter, or of up to 64 named groups under it, from the exact Mutations scan and the
// consensus call on the device (K15), with its parser.  No counterpart in the reference.
namespace {

/// The rows of one group on one partition: how many, and their bitset (nullptr: every row of the partition).
struct GroupRows {
   uint32_t cardinality;
   const uint64_t* bits;
};

/// `expression` (nullptr: no expression, the base alone) AND the base — the rows of the query's filter on this partition, of which
/// there are base_selected > 0, base_bits == nullptr where they are all rows.  Compiled as evaluateSubFilter compiles; the AND is an
/// Intersection with the base's bitset as a stored column, so one fused launch yields the bitset and its cardinality.  A bitset
/// made here is kept in `live`.  `owner` opens the message when the expression does not compile.
GroupRows evaluateWithinBase(
   const Database& database, const DatabasePartition& partition, const filter_expressions::Expression* expression, uint32_t base_selected,
   const uint64_t* base_bits, LiveSet& live, const std::string& owner
) {
   if (expression == nullptr) {
      return {base_selected, base_bits};
   }
   std::unique_ptr<operators::Operator> root;
   try {
      root = expression->compile(database, partition, filter_expressions::Expression::AmbiguityMode::NONE);
   } catch (const QueryParseException& error) {
      throw QueryParseException(owner + " is not a valid filter expression: " + error.what());
   }
   if (root->type() == operators::EMPTY) {
      return {0, nullptr};
   }
   if (root->type() == operators::FULL) {
      return {base_selected, base_bits};
   }
   if (base_bits != nullptr) {
      const RowSpace rows = root->rows;
      operators::OperatorVector children;
      children.push_back(std::move(root));
      children.push_back(std::make_unique<operators::IndexScan>(base_bits, rows));
      root = std::make_unique<operators::Intersection>(std::move(children), operators::OperatorVector{}, rows);
   }
   OperatorResult result = operators::Operator::evaluate(std::move(root));
   result.materialize();  // one launch yields both the bitset and its cardinality
   const uint32_t cardinality = result.cardinality();
   if (cardinality == 0 || cardinality == partition.sequence_count) {
      return {cardinality, nullptr};
   }
   return {cardinality, live.keep(std::move(result))};
}

/// A group of Consensus / MutationsComparison: what messages call it and its expression (nullptr: the query's filter alone).
struct GroupFilter {
   std::string name;
   const filter_expressions::Expression* filter;
};

/// The exact Mutations tables of the groups of a request, on the device, with what the launches into them read.  Declared before the
/// launchAndWait that fills and reads it: nothing in it returns to the pool before the stream has been waited for.
struct GroupTables {
   std::vector<uint32_t> group_rows;          // the rows of every group, over all partitions
   DeviceBuffer tables;                       // a table per group, back to back: it never leaves the device.  None: nothing to scan
   const uint8_t* reference_index = nullptr;  // the reference's symbol index of every position, on the device
   DeviceBuffer own_reference;                // only where the database keeps no reference index on the device
   LiveSet live;                              // the groups' bitsets of one partition at a time
};

/// Fills `out` for the sequence store `name` (inside a launchAndWait): the pooled tables cleared once; per partition whose base
/// filter selects a row, every group's rows within the base (evaluateWithinBase), the store's cached totals added for a group that is
/// every row of the partition (a NULL filter: no pass over the planes) and ONE exact silo_gpu_mutations_scan_batch for the others;
/// then the reference index.  Where the database has no partition or the sequence no position, only the groups' rows are counted.
template <typename SymbolType>
void fillGroupTables(
   const Database& database, const std::vector<OperatorResult>& bitmap_filter, const std::string& name, const std::vector<GroupFilter>& groups,
   const std::string& action_name, GroupTables& out
) {
   const auto& reference = database.getSequenceStores<SymbolType>().at(name).reference_sequence;
   constexpr uint32_t n_symbols = SymbolType::VALID_MUTATION_SYMBOLS.size();
   const auto positions = static_cast<uint32_t>(reference.size());
   const auto n_groups = static_cast<uint32_t>(groups.size());
   const size_t table_words = static_cast<size_t>(positions) * n_symbols;  // of one group
   const bool on_device = !database.partitions.empty() && positions != 0;
   out.group_rows.assign(n_groups, 0);
   if (on_device) {
      out.tables = database.partitions.front().pool.acquire(n_groups * table_words * sizeof(uint32_t));
      checkGpu(silo_gpu_memset_async(out.tables.get(), 0, n_groups * table_words * sizeof(uint32_t), queryStream()), "silo_gpu_memset_async");
   }
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      const OperatorResult& filter = bitmap_filter[partition_id];
      const uint32_t base_selected = partition.sequence_count == 0 ? 0 : filter.cardinality();
      if (base_selected == 0) {
         continue;
      }
      // a filter that selects every row is passed as NULL (no all-ones bitset is made for it)
      const uint64_t* base_bits = base_selected == partition.sequence_count ? nullptr : filter.bitset();
      out.live.waitAndRelease();  // the scans of the partition before may still read its groups' bitsets
      const SequenceStorePartition<SymbolType>& store = partition.getSequenceStores<SymbolType>().at(name);
      std::vector<const uint64_t*> scan_filters;  // the groups that select some rows of the partition, not all
      std::vector<uint32_t*> scan_tables;
      for (uint32_t g = 0; g < n_groups; ++g) {
         const std::string owner = action_name + " action: the field filterExpression of the group '" + groups[g].name + "'";
         const GroupRows rows = evaluateWithinBase(database, partition, groups[g].filter, base_selected, base_bits, out.live, owner);
         out.group_rows[g] += rows.cardinality;
         if (rows.cardinality == 0 || !on_device) {  // empty here: its table stays as it is
            continue;
         }
         uint32_t* table = out.tables.as<uint32_t>() + g * table_words;
         if (rows.bits == nullptr) {  // every row: the store's cached totals are added, no pass over the planes
            checkGpu(silo_gpu_mutations_scan(store.store, store.seqstore_id, nullptr, 0, positions, table, queryStream()), "silo_gpu_mutations_scan");
            out.live.launched();
         } else {
            scan_filters.push_back(rows.bits);
            scan_tables.push_back(table);
         }
      }
      if (!scan_filters.empty()) {
         // the EXACT scan (never a min_proportion variant: a pruned group would land on the derived symbol), every plane row
         // read once per SILO_GPU_MAX_SCAN_BATCH groups; it accumulates, so partitions sum as they do for Mutations
         checkGpu(
            silo_gpu_mutations_scan_batch(
               store.store, store.seqstore_id, scan_filters.data(), static_cast<uint32_t>(scan_filters.size()), 0, positions, scan_tables.data(),
               queryStream()
            ),
            "silo_gpu_mutations_scan_batch"
         );
         out.live.launched();
      }
   }
   if (on_device) {
      const MutationTableLayout& layout = database.getMutationTableLayout<SymbolType>();
      if (layout.reference_index_device != nullptr) {
         out.reference_index = layout.reference_index_device.get() + layout.position_offset.at(name);
      } else {
         std::vector<uint8_t> index(positions, 0xFF);
         for (uint32_t p = 0; p < positions; ++p) {
            for (size_t s = 0; s < n_symbols; ++s) {
               if (SymbolType::VALID_MUTATION_SYMBOLS[s] == reference[p]) {
                  index[p] = static_cast<uint8_t>(s);
               }
            }
         }
         out.own_reference = database.partitions.front().pool.acquire(positions);
         checkGpu(silo_gpu_memcpy_h2d(out.own_reference.get(), index.data(), positions, queryStream()), "silo_gpu_memcpy_h2d");
         out.reference_index = out.own_reference.as<uint8_t>();
      }
   }
}

}  // namespace

template <typename SymbolType>
void Consensus<SymbolType>::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"name", "count", "ambiguousPositions", "lowCoveragePositions", "deletedPositions", "differences"});
}

template <typename SymbolType>
QueryResult Consensus<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = actionName();
   requireUnsharded(database, action_name);
   const auto [name, store] = sequenceStoreOf<SymbolType>(
      database, sequence_name, "Database does not contain the " + std::string(SymbolType::SYMBOL_NAME_LOWER_CASE) + " sequence with name: "
   );
   constexpr uint32_t summary_words = 4;  // ambiguous, low coverage, deleted, differences
   const auto positions = static_cast<uint32_t>(store.reference_sequence.size());
   const auto n_groups = static_cast<uint32_t>(groups.size());
   const char missing = SymbolType::symbolToChar(SymbolType::SYMBOL_MISSING);

   // what a group nobody scanned gets: the missing symbol everywhere, every position low coverage
   std::vector<uint32_t> summary(static_cast<size_t>(n_groups) * summary_words, 0);
   std::string characters(static_cast<size_t>(n_groups) * positions, missing);
   for (uint32_t g = 0; g < n_groups; ++g) {
      summary[g * summary_words + 1] = positions;
   }
   std::vector<GroupFilter> group_filters;
   for (const Group& group : groups) {
      group_filters.push_back({group.name.value_or(""), group.filter.get()});
   }
   // nothing in here returns to the pool before the stream has been waited for: the launches read it
   GroupTables tables;
   DeviceBuffer device_result;  // the summaries, then the characters: the one thing fetched
   launchAndWait([&] {
      fillGroupTables<SymbolType>(database, bitmap_filter, name, group_filters, action_name, tables);
      if (tables.tables) {
         device_result = database.partitions.front().pool.acquire(summary.size() * sizeof(uint32_t) + characters.size());
         auto* device_summary = device_result.as<uint32_t>();
         char* device_characters = device_result.as<char>() + summary.size() * sizeof(uint32_t);
         checkGpu(
            silo_gpu_consensus_call(
               SymbolType::ABI_ALPHABET, tables.tables.as<uint32_t>(), n_groups, positions, tables.reference_index, threshold, min_depth,
               device_characters, device_summary, queryStream()
            ),
            "silo_gpu_consensus_call"
         );
         HostFetch fetch(device_result.get(), summary.size() * sizeof(uint32_t) + characters.size(), queryStream());
         const auto* host = static_cast<const char*>(fetch.wait());
         std::memcpy(summary.data(), host, summary.size() * sizeof(uint32_t));
         characters.assign(host + summary.size() * sizeof(uint32_t), characters.size());
      }
   });
   const std::vector<uint32_t>& group_rows = tables.group_rows;

   // what came off the device is checked before it becomes a row: every character one the rule can give, the three kinds of
   // position disjoint
   const std::string_view callable = std::is_same_v<SymbolType, Nucleotide> ? std::string_view("-ACGTMRWSYKVHDBN") : std::string_view("-ACDEFGHIKLMNPQRSTVWY*X");
   QueryResult results;
   results.query_result.reserve(n_groups);
   for (uint32_t g = 0; g < n_groups; ++g) {
      const std::string consensus = characters.substr(static_cast<size_t>(g) * positions, positions);
      const uint32_t* sums = summary.data() + static_cast<size_t>(g) * summary_words;
      if (consensus.find_first_not_of(callable) != std::string::npos) {
         throw std::runtime_error(action_name + ": the device called a character that no call can be");
      }
      if (static_cast<uint64_t>(sums[0]) + sums[1] + sums[2] > positions || sums[3] > positions) {
         throw std::runtime_error(action_name + ": the device counted more ambiguous, low-coverage and deleted positions than there are positions");
      }
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("name", groups[g].name.has_value() ? JsonValue{*groups[g].name} : JsonValue{std::nullopt});
      entry.fields.emplace("sequenceName", name);
      entry.fields.emplace("count", static_cast<int32_t>(group_rows[g]));
      entry.fields.emplace("consensus", consensus);
      entry.fields.emplace("ambiguousPositions", static_cast<int32_t>(sums[0]));
      entry.fields.emplace("lowCoveragePositions", static_cast<int32_t>(sums[1]));
      entry.fields.emplace("deletedPositions", static_cast<int32_t>(sums[2]));
      entry.fields.emplace("differences", static_cast<int32_t>(sums[3]));
   }
   return results;
}

template class Consensus<Nucleotide>;
template class Consensus<AminoAcid>;

// ---- MutationsComparison -----------------------------------------------------------------------------------
// The mutations that up to 64 named groups under the query's filter carry, with every group's count and coverage, from the exact
// Mutations scan of the groups and the comparison on the device (K17), with its parser.  No counterpart in the reference.
namespace {

/// K4's bound (k_mutations_select, Mutations' own row selection): a count passes a coverage above 0 iff it is above this.
uint32_t mustExceed(uint32_t coverage, double min_proportion) {
   return min_proportion == 0 ? 0 : static_cast<uint32_t>(std::ceil(static_cast<double>(coverage) * min_proportion) - 1);
}

}  // namespace

template <typename SymbolType>
void MutationsComparison<SymbolType>::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"mutation", "position", "group", "count", "coverage", "proportion", "difference"});
}

template <typename SymbolType>
QueryResult MutationsComparison<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = actionName();
   requireUnsharded(database, action_name);
   const auto [name, store] = sequenceStoreOf<SymbolType>(
      database, sequence_name, "Database does not contain the " + std::string(SymbolType::SYMBOL_NAME_LOWER_CASE) + " sequence with name: "
   );
   const auto& reference = store.reference_sequence;
   constexpr uint32_t n_symbols = SymbolType::VALID_MUTATION_SYMBOLS.size();
   constexpr size_t header_words = 4;
   const auto positions = static_cast<uint32_t>(reference.size());
   const auto n_groups = static_cast<uint32_t>(groups.size());
   const size_t record_words = 2 + static_cast<size_t>(n_groups) * 2;  // {position, symbol}, and {count, coverage} of every group

   std::vector<GroupFilter> group_filters;
   for (const Group& group : groups) {
      group_filters.push_back({group.name, group.filter.get()});
   }
   uint32_t n_records = 0;
   std::vector<uint32_t> records;  // n_records x {position, symbol}, then n_records x n_groups x {count, coverage}: as they came
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read and write it
      GroupTables tables;
      DeviceBuffer device_out[2];  // of the first comparison and, where its capacity was too low, of the second
      launchAndWait([&] {
         fillGroupTables<SymbolType>(database, bitmap_filter, name, group_filters, action_name, tables);
         if (!tables.tables) {
            return;
         }
         uint32_t capacity = FIRST_CAPACITY;
         for (size_t call = 0; call < 2; ++call) {
            DeviceBuffer& out = device_out[call];
            out = database.partitions.front().pool.acquire((header_words + capacity * record_words) * sizeof(uint32_t));
            checkGpu(
               silo_gpu_mutations_compare(
                  SymbolType::ABI_ALPHABET, tables.tables.as<uint32_t>(), n_groups, positions, tables.reference_index, min_proportion, min_difference,
                  capacity, out.as<uint32_t>(), queryStream()
               ),
               "silo_gpu_mutations_compare"
            );
            const HostFetch header(out.get(), header_words * sizeof(uint32_t), queryStream());
            const uint32_t selected = *static_cast<const uint32_t*>(header.wait());
            if (selected > capacity) {
               if (call == 1) {  // the tables have not changed: the second count is the first
                  throw std::runtime_error(action_name + ": the device selected " + std::to_string(selected) + " cells where it had selected " + std::to_string(capacity));
               }
               capacity = selected;  // exactly as many: the count is deterministic
               continue;
            }
            n_records = selected;
            if (selected != 0) {
               // one copy from the first record to the last cell in use (the record slots nobody took lie between them)
               const size_t words = static_cast<size_t>(capacity) * 2 + static_cast<size_t>(selected) * n_groups * 2;
               const HostFetch fetch(out.as<uint32_t>() + header_words, words * sizeof(uint32_t), queryStream());
               const auto* host = static_cast<const uint32_t*>(fetch.wait());
               records.assign(host, host + static_cast<size_t>(selected) * 2);
               records.insert(records.end(), host + static_cast<size_t>(capacity) * 2, host + words);
            }
            break;
         }
      });
   }

   // what came off the device is checked before it becomes rows: every record a cell of the table that is not the reference's, once,
   // with counts that a coverage can hold, and selected by the rule as the host computes it
   const auto broken = [&](const std::string& what) { return std::runtime_error(action_name + ": the device delivered " + what); };
   const uint32_t* cells = records.data() + static_cast<size_t>(n_records) * 2;
   std::vector<uint32_t> order(n_records);
   for (uint32_t r = 0; r < n_records; ++r) {
      order[r] = r;
      if (records[r * 2] >= positions || records[r * 2 + 1] >= n_symbols) {
         throw broken("a record outside the table");
      }
   }
   const auto key = [&](uint32_t r) { return static_cast<uint64_t>(records[r * 2]) * n_symbols + records[r * 2 + 1]; };
   std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
   QueryResult results;
   results.query_result.reserve(static_cast<size_t>(n_records) * n_groups);
   for (uint32_t k = 0; k < n_records; ++k) {
      const uint32_t r = order[k];
      const uint32_t position = records[r * 2];
      const uint32_t symbol = records[r * 2 + 1];
      const uint32_t* of_groups = cells + static_cast<size_t>(r) * n_groups * 2;
      if (k != 0 && key(order[k - 1]) == key(r)) {
         throw broken("a record twice");
      }
      if (SymbolType::VALID_MUTATION_SYMBOLS[symbol] == reference[position]) {
         throw broken("the reference's symbol as a mutation");
      }
      bool passes = false;
      uint32_t covered = 0;
      double highest = 0;
      double lowest = 1;
      for (uint32_t g = 0; g < n_groups; ++g) {
         const uint32_t count = of_groups[g * 2];
         const uint32_t coverage = of_groups[g * 2 + 1];
         if (count > coverage) {
            throw broken("a count above its coverage");
         }
         if (coverage != 0) {
            const double proportion = static_cast<double>(count) / static_cast<double>(coverage);
            ++covered;
            passes = passes || count > mustExceed(coverage, min_proportion);
            highest = std::max(highest, proportion);
            lowest = std::min(lowest, proportion);
         }
      }
      const double difference = covered >= 2 ? highest - lowest : 0.0;
      if (!passes || !(difference >= min_difference)) {
         throw broken("a record that the rule does not select");
      }
      const std::string mutation =
         SymbolType::symbolToChar(reference[position]) + std::to_string(position + 1) + SymbolType::symbolToChar(SymbolType::VALID_MUTATION_SYMBOLS[symbol]);
      for (uint32_t g = 0; g < n_groups; ++g) {
         const uint32_t count = of_groups[g * 2];
         const uint32_t coverage = of_groups[g * 2 + 1];
         QueryResultEntry& entry = results.query_result.emplace_back();
         entry.fields.emplace("mutation", mutation);
         entry.fields.emplace("sequenceName", name);
         entry.fields.emplace("position", static_cast<int32_t>(position + 1));
         entry.fields.emplace("group", groups[g].name);
         entry.fields.emplace("count", static_cast<int32_t>(count));
         entry.fields.emplace("coverage", static_cast<int32_t>(coverage));
         entry.fields.emplace("proportion", coverage != 0 ? JsonValue{static_cast<double>(count) / static_cast<double>(coverage)} : JsonValue{std::nullopt});
         entry.fields.emplace("difference", difference);
      }
   }
   return results;
}

template class MutationsComparison<Nucleotide>;
template class MutationsComparison<AminoAcid>;

// ---- MeanDistances -------------------------------------------------------------------------------------------
// The sums of the pairwise distances within and between up to 64 groups under the query's filter in up to 256 regions of a sequence,
// from the exact Mutations scan of the groups and the sums over their tables on the device (K24).  No counterpart in the reference.
namespace {

using Wide = unsigned __int128;  // a sum over pairs of rows and positions: (2^32)^2 pairs x 2^32 positions

std::string decimal(Wide value) {
   std::string digits;
   do {
      digits.push_back(static_cast<char>('0' + static_cast<int>(value % 10)));
      value /= 10;
   } while (value != 0);
   return {digits.rbegin(), digits.rend()};
}

/// One IEEE division of the correctly rounded doubles of the two integers; null where the divisor is 0.
JsonValue ratio(Wide dividend, Wide divisor) {
   if (divisor == 0) {
      return std::nullopt;
   }
   return static_cast<double>(dividend) / static_cast<double>(divisor);
}

}  // namespace

template <typename SymbolType>
void MeanDistances<SymbolType>::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"region", "positionFrom", "positionTo", "group", "otherGroup", "count", "otherCount", "segregatingSites", "fixedDifferences",
                       "meanDistance", "meanCompared", "distancePerSite"});
}

template <typename SymbolType>
QueryResult MeanDistances<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = actionName();
   requireUnsharded(database, action_name);
   const auto [name, store] = sequenceStoreOf<SymbolType>(
      database, sequence_name, "Database does not contain the " + std::string(SymbolType::SYMBOL_NAME_LOWER_CASE) + " sequence with name: "
   );
   constexpr size_t record_words = SILO_GPU_PAIR_SUM_WORDS;
   const auto positions = static_cast<uint32_t>(store.reference_sequence.size());
   const auto n_groups = static_cast<uint32_t>(groups.size());
   const size_t n_pairs = static_cast<size_t>(n_groups) * (n_groups + 1) / 2;
   std::vector<uint32_t> ranges;  // {first, end} of every region, as K24 takes them
   for (const Region& region : regions) {
      const uint32_t end = region.name.has_value() ? region.end : positions;
      CHECK_SILO_QUERY(
         end <= positions, action_name + ": the region '" + region.name.value_or("") + "': positionTo " + std::to_string(end) +
                              " is past the end of the sequence '" + name + "' (" + std::to_string(positions) + " positions)"
      )
      ranges.insert(ranges.end(), {region.first, end});
   }
   std::vector<GroupFilter> group_filters;
   for (const Group& group : groups) {
      group_filters.push_back({group.name.value_or(""), group.filter.get()});
   }
   // what groups that nobody scanned get: no pair compared anywhere
   std::vector<uint64_t> records(regions.size() * n_pairs * record_words, 0);
   // nothing in here returns to the pool before the stream has been waited for: the launches read and write it
   GroupTables tables;
   DeviceBuffer device_records;
   launchAndWait([&] {
      fillGroupTables<SymbolType>(database, bitmap_filter, name, group_filters, action_name, tables);
      if (tables.tables) {
         device_records = database.partitions.front().pool.acquire(records.size() * sizeof(uint64_t));
         checkGpu(
            silo_gpu_table_pair_sums(
               SymbolType::ABI_ALPHABET, tables.tables.as<uint32_t>(), n_groups, positions, ranges.data(), static_cast<uint32_t>(regions.size()),
               device_records.as<uint64_t>(), queryStream()
            ),
            "silo_gpu_table_pair_sums"
         );
         const HostFetch fetch(device_records.get(), records.size() * sizeof(uint64_t), queryStream());
         std::memcpy(records.data(), fetch.wait(), records.size() * sizeof(uint64_t));
      }
   });
   const std::vector<uint32_t>& group_rows = tables.group_rows;

   // what came off the device is checked before it becomes a row: no more differing pairs than compared ones, no more compared ones
   // than pairs of rows and positions, no more sites than positions
   const auto broken = [&](const std::string& what) { return std::runtime_error(action_name + ": the device delivered " + what); };
   const auto nameOf = [](const Group& group) { return group.name.has_value() ? JsonValue{*group.name} : JsonValue{std::nullopt}; };
   QueryResult results;
   results.query_result.reserve(regions.size() * (between ? n_pairs : n_groups));
   for (size_t r = 0; r < regions.size(); ++r) {
      const uint32_t first = ranges[2 * r];
      const uint32_t length = ranges[2 * r + 1] - first;
      const uint64_t* of_region = records.data() + r * n_pairs * record_words;
      for (uint32_t g = 0; g < n_groups; ++g) {
         for (uint32_t h = g; h < n_groups; ++h, of_region += record_words) {
            if (g != h && !between) {
               continue;
            }
            const Wide differences = (static_cast<Wide>(of_region[1]) << 64) | of_region[0];
            const Wide compared = (static_cast<Wide>(of_region[3]) << 64) | of_region[2];
            const uint64_t sites = of_region[4];
            const Wide pairs = g == h ? static_cast<Wide>(group_rows[g]) * (group_rows[g] == 0 ? 0 : group_rows[g] - 1) / 2
                                      : static_cast<Wide>(group_rows[g]) * group_rows[h];
            if (differences > compared) {
               throw broken("more differing pairs than compared ones");
            }
            if (compared > pairs * length) {
               throw broken("more compared pairs than there are pairs of rows and positions");
            }
            if (sites > length) {
               throw broken("more sites than the region has positions");
            }
            if (compared == 0 && differences != 0) {
               throw broken("differences where nothing was compared");
            }
            QueryResultEntry& entry = results.query_result.emplace_back();
            entry.fields.emplace("region", regions[r].name.has_value() ? JsonValue{*regions[r].name} : JsonValue{std::nullopt});
            entry.fields.emplace("positionFrom", static_cast<int32_t>(first + 1u));
            entry.fields.emplace("positionTo", static_cast<int32_t>(first + length));
            entry.fields.emplace("sequenceName", name);
            entry.fields.emplace("group", nameOf(groups[g]));
            entry.fields.emplace("otherGroup", nameOf(groups[h]));
            entry.fields.emplace("count", static_cast<int32_t>(group_rows[g]));
            entry.fields.emplace("otherCount", static_cast<int32_t>(group_rows[h]));
            entry.fields.emplace("pairs", decimal(pairs));
            entry.fields.emplace("differences", decimal(differences));
            entry.fields.emplace("comparedPositions", decimal(compared));
            entry.fields.emplace("segregatingSites", g == h ? JsonValue{static_cast<int32_t>(sites)} : JsonValue{std::nullopt});
            entry.fields.emplace("fixedDifferences", g != h ? JsonValue{static_cast<int32_t>(sites)} : JsonValue{std::nullopt});
            entry.fields.emplace("meanDistance", ratio(differences, pairs));
            entry.fields.emplace("meanCompared", ratio(compared, pairs));
            entry.fields.emplace("distancePerSite", ratio(differences, compared));
         }
      }
   }
   return results;
}

template class MeanDistances<Nucleotide>;
template class MeanDistances<AminoAcid>;

// ---- JSON -> the three actions ---------------------------------------------------------------------------
namespace {

/// One entry of the mutations field of MutationsOverTime: [<sequenceName>:][<reference symbol>]<1-based position><symbol>.
template <typename SymbolType>
typename MutationsOverTime<SymbolType>::Mutation parseOverTimeMutation(const std::string& text, const std::string& action_name) {
   const std::string invalid = "The mutation '" + text + "' of " + action_name + " is not of the form [<sequenceName>:][<reference symbol>]<position><symbol>";
   typename MutationsOverTime<SymbolType>::Mutation mutation{};
   std::string rest = text;
   if (const size_t colon = text.rfind(':'); colon != std::string::npos) {
      mutation.sequence_name = text.substr(0, colon);
      rest = text.substr(colon + 1);
   }
   CHECK_SILO_QUERY(
      (std::is_same_v<SymbolType, Nucleotide>) || mutation.sequence_name.has_value(),
      "The mutation '" + text + "' of " + action_name + " must name its gene: <sequenceName>:[<reference symbol>]<position><symbol>"
   )
   size_t first_digit = 0;
   if (!rest.empty() && (rest[0] < '0' || rest[0] > '9')) {
      mutation.reference_symbol = rest[0];
      first_digit = 1;
   }
   size_t end = first_digit;
   while (end < rest.size() && rest[end] >= '0' && rest[end] <= '9') {
      ++end;
   }
   CHECK_SILO_QUERY(end > first_digit && end - first_digit <= 9 && end + 1 == rest.size(), invalid)
   mutation.position = static_cast<uint32_t>(std::stoul(rest.substr(first_digit, end - first_digit)));
   const auto symbol = SymbolType::charToSymbol(rest[end]);
   const bool valid = symbol.has_value() &&
                      std::find(SymbolType::VALID_MUTATION_SYMBOLS.begin(), SymbolType::VALID_MUTATION_SYMBOLS.end(), *symbol) != SymbolType::VALID_MUTATION_SYMBOLS.end();
   CHECK_SILO_QUERY(valid, "The symbol '" + std::string(1, rest[end]) + "' of the mutation '" + text + "' of " + action_name + " is not a valid mutation symbol")
   mutation.symbol = *symbol;
   return mutation;
}

/// The dateField and dateRanges fields of the over-time actions: the column's name and the ranges in request order (validated:
/// at most SILO_GPU_MAX_DATE_RANGES, valid dates, dateFrom <= dateTo, pairwise disjoint with both ends inclusive).
std::pair<std::string, std::vector<OverTimeDateRange>> parseDateFieldAndRanges(const json::Value& json, const std::string& action_name) {
   CHECK_SILO_QUERY(
      json.contains("dateField") && json["dateField"].is_string(), action_name + " action must contain the field dateField of type string"
   )
   CHECK_SILO_QUERY(
      json.contains("dateRanges") && json["dateRanges"].is_array(),
      action_name + " action must contain the field dateRanges: an array of objects {\"dateFrom\": string or null, \"dateTo\": string or null}"
   )
   std::vector<OverTimeDateRange> ranges;
   for (const auto& element : json["dateRanges"].items()) {
      CHECK_SILO_QUERY(
         element.is_object(), action_name + " action: every entry of dateRanges must be an object {\"dateFrom\": string or null, \"dateTo\": string or null}"
      )
      CHECK_SILO_QUERY(
         ranges.size() < SILO_GPU_MAX_DATE_RANGES, action_name + " action takes at most " + std::to_string(SILO_GPU_MAX_DATE_RANGES) + " date ranges"
      )
      OverTimeDateRange range;
      for (const char* field : {"dateFrom", "dateTo"}) {
         if (!element.contains(field) || element[field].is_null()) {
            continue;
         }
         CHECK_SILO_QUERY(element[field].is_string(), action_name + " action: the field " + field + " of a date range must be a string or null")
         const common::Date date = common::stringToDate(element[field].as_string());
         CHECK_SILO_QUERY(date != common::NULL_DATE, action_name + " action: the " + field + " '" + element[field].as_string() + "' is not a valid date (YYYY-MM-DD)")
         (std::string_view(field) == "dateFrom" ? range.from : range.to) = date;
      }
      CHECK_SILO_QUERY(
         !range.from.has_value() || !range.to.has_value() || *range.from <= *range.to,
         action_name + " action: a date range has dateFrom after dateTo: " + element.dump()
      )
      ranges.push_back(range);
   }
   // pairwise disjoint (both ends inclusive): in order of their start, each must begin after the one before ends
   std::vector<std::pair<common::Date, common::Date>> spans;
   for (const auto& range : ranges) {
      spans.emplace_back(range.from.value_or(common::Date{0}), range.to.value_or(common::Date{UINT32_MAX}));
   }
   std::sort(spans.begin(), spans.end());
   for (size_t k = 1; k < spans.size(); ++k) {
      CHECK_SILO_QUERY(spans[k].first > spans[k - 1].second, action_name + " action: the date ranges overlap; each row may fall in at most one")
   }
   return {json["dateField"].as_string(), std::move(ranges)};
}

/// One entry of a list of labelled queries (`list`: the field that holds the list): an object, below the list's limit
/// (`limit_message` otherwise), with a string displayLabel that no entry of the list had before.  Returns the label.
std::string parseLabelledEntry(
   const json::Value& element, const std::string& action_name, const std::string& list, const std::string& entry_form, bool below_limit,
   const std::string& limit_message, std::set<std::string>& labels
) {
   CHECK_SILO_QUERY(element.is_object(), action_name + " action: every entry of " + list + " must be an object " + entry_form)
   CHECK_SILO_QUERY(below_limit, limit_message)
   CHECK_SILO_QUERY(
      element.contains("displayLabel") && element["displayLabel"].is_string(),
      action_name + " action: every entry of " + list + " must contain the field displayLabel of type string"
   )
   const std::string label = element["displayLabel"].as_string();
   CHECK_SILO_QUERY(labels.insert(label).second, action_name + " action: the displayLabel '" + label + "' occurs more than once in " + list)
   return label;
}

/// The sub-expressions of a request: those with the same JSON text are parsed once and share an index.
struct DistinctFilters {
   filter_expressions::ExpressionVector filters;
   std::map<std::string, uint32_t> index_of_text;

   /// The index of the filter expression in `field` of a labelled entry; `owner` is what messages call the entry.
   uint32_t parse(const json::Value& element, const char* field, const std::string& action_name, const std::string& owner) {
      CHECK_SILO_QUERY(
         element.contains(field) && element[field].is_object(),
         action_name + " action: " + owner + " must contain the field " + field + " of type object (a filter expression)"
      )
      const auto [found, is_new] = index_of_text.emplace(element[field].dump(), static_cast<uint32_t>(filters.size()));
      if (is_new) {
         try {
            filters.push_back(filter_expressions::parseExpression(element[field]));
         } catch (const QueryParseException& ex) {
            throw QueryParseException(action_name + " action: the field " + field + " of " + owner + " is not a valid filter expression: " + ex.what());
         }
      }
      return found->second;
   }
};

}  // namespace

/// An entry of the groups field of Consensus, MutationsComparison and MeanDistances, as the messages show it.
const std::string GROUP_ENTRY_FORM = "{\"name\": string, \"filterExpression\": filter expression}";

/// The entries of a groups field (`list`, an array) in request order: objects with a string name that no entry before had and a
/// filterExpression, whose own complaint comes behind the field and the group.
std::vector<std::pair<std::string, std::unique_ptr<filter_expressions::Expression>>> parseGroupEntries(const json::Value& list, const std::string& action_name) {
   std::vector<std::pair<std::string, std::unique_ptr<filter_expressions::Expression>>> groups;
   std::set<std::string> names;
   for (const auto& element : list.items()) {
      CHECK_SILO_QUERY(element.is_object(), action_name + " action: every entry of groups must be an object " + GROUP_ENTRY_FORM)
      CHECK_SILO_QUERY(
         element.contains("name") && element["name"].is_string(), action_name + " action: every entry of groups must contain the field name of type string"
      )
      const std::string group_name = element["name"].as_string();
      CHECK_SILO_QUERY(names.insert(group_name).second, action_name + " action: the name '" + group_name + "' occurs more than once in groups")
      const std::string owner = action_name + " action: the field filterExpression of the group '" + group_name + "'";
      CHECK_SILO_QUERY(element.contains("filterExpression") && element["filterExpression"].is_object(), owner + " must be of type object (a filter expression)")
      try {
         groups.emplace_back(group_name, filter_expressions::parseExpression(element["filterExpression"]));
      } catch (const QueryParseException& error) {
         throw QueryParseException(owner + " is not a valid filter expression: " + error.what());
      }
   }
   return groups;
}

template <typename SymbolType>
std::unique_ptr<Action> parseMutationsOverTime(const json::Value& json) {
   using OverTime = MutationsOverTime<SymbolType>;
   const std::string action_name = std::is_same_v<SymbolType, Nucleotide> ? "MutationsOverTime" : "AminoAcidMutationsOverTime";
   CHECK_SILO_QUERY(
      json.contains("mutations") && json["mutations"].is_array(), action_name + " action must contain the field mutations of type array of strings"
   )
   std::vector<typename OverTime::Mutation> mutations;
   for (const auto& element : json["mutations"].items()) {
      CHECK_SILO_QUERY(element.is_string(), action_name + " action must contain the field mutations of type array of strings, found " + element.dump())
      CHECK_SILO_QUERY(
         mutations.size() < OverTime::MAX_MUTATIONS, action_name + " action takes at most " + std::to_string(OverTime::MAX_MUTATIONS) + " mutations"
      )
      mutations.push_back(parseOverTimeMutation<SymbolType>(element.as_string(), action_name));
   }
   auto [date_field, ranges] = parseDateFieldAndRanges(json, action_name);
   return std::make_unique<OverTime>(std::move(mutations), std::move(date_field), std::move(ranges));
}

template std::unique_ptr<Action> parseMutationsOverTime<Nucleotide>(const json::Value& json);
template std::unique_ptr<Action> parseMutationsOverTime<AminoAcid>(const json::Value& json);

std::unique_ptr<Action> parseQueriesOverTime(const json::Value& json) {
   const std::string action_name = "QueriesOverTime";
   const std::string entry_form = "{\"displayLabel\": string, \"countQuery\": filter expression, \"coverageQuery\": filter expression}";
   CHECK_SILO_QUERY(
      json.contains("queries") && json["queries"].is_array(), action_name + " action must contain the field queries: an array of objects " + entry_form
   )
   std::vector<QueriesOverTime::LabelledQuery> queries;
   DistinctFilters distinct;  // sub-expressions with the same JSON text share a row of the table
   std::set<std::string> labels;
   for (const auto& element : json["queries"].items()) {
      const std::string label = parseLabelledEntry(
         element, action_name, "queries", entry_form, queries.size() < QueriesOverTime::MAX_QUERIES,
         action_name + " action takes at most " + std::to_string(QueriesOverTime::MAX_QUERIES) + " queries", labels
      );
      const std::string owner = "the query '" + label + "'";
      const uint32_t count_filter = distinct.parse(element, "countQuery", action_name, owner);
      const uint32_t coverage_filter = distinct.parse(element, "coverageQuery", action_name, owner);
      queries.push_back({label, count_filter, coverage_filter});
   }
   auto [date_field, ranges] = parseDateFieldAndRanges(json, action_name);
   return std::make_unique<QueriesOverTime>(std::move(queries), std::move(distinct.filters), std::move(date_field), std::move(ranges));
}

std::unique_ptr<Action> parseCrossTabulation(const json::Value& json) {
   const std::string action_name = "CrossTabulation";
   const std::string entry_form = "{\"displayLabel\": string, \"query\": filter expression}";
   CHECK_SILO_QUERY(
      json.contains("rowQueries") && json["rowQueries"].is_array(), action_name + " action must contain the field rowQueries: an array of objects " + entry_form
   )
   CHECK_SILO_QUERY(
      !json.contains("columnQueries") || json["columnQueries"].is_array(),
      action_name + " action: the field columnQueries, if present, must be an array of objects " + entry_form
   )
   DistinctFilters distinct;  // sub-expressions with the same JSON text, in either list, are parsed once
   const auto parseList = [&](const std::string& list, std::vector<CrossTabulation::LabelledQuery>& queries, std::vector<uint32_t>& side) {
      std::set<std::string> labels;
      std::map<uint32_t, uint32_t> slot_of_filter;
      for (const auto& element : json[list].items()) {
         const std::string label = parseLabelledEntry(
            element, action_name, list, entry_form, queries.size() < CrossTabulation::MAX_QUERIES,
            action_name + " action takes at most " + std::to_string(CrossTabulation::MAX_QUERIES) + " entries in " + list, labels
         );
         const uint32_t filter = distinct.parse(element, "query", action_name, "the entry '" + label + "' of " + list);
         const auto [slot, first_use] = slot_of_filter.emplace(filter, static_cast<uint32_t>(side.size()));
         if (first_use) {
            side.push_back(filter);
         }
         queries.push_back({label, slot->second});
      }
   };
   std::vector<CrossTabulation::LabelledQuery> row_queries, column_queries;
   std::vector<uint32_t> row_filters, column_filters;
   parseList("rowQueries", row_queries, row_filters);
   if (json.contains("columnQueries")) {
      parseList("columnQueries", column_queries, column_filters);
   } else {  // the co-occurrence matrix of the row queries
      column_queries = row_queries;
      column_filters = row_filters;
   }
   CHECK_SILO_QUERY(
      row_queries.size() * column_queries.size() <= CrossTabulation::MAX_CELLS,
      action_name + " action: " + std::to_string(row_queries.size()) + " rowQueries x " + std::to_string(column_queries.size()) +
         (json.contains("columnQueries") ? " columnQueries" : " columnQueries (the rowQueries again)") + " are more than the " +
         std::to_string(CrossTabulation::MAX_CELLS) + " cells a response may hold"
   )
   return std::make_unique<CrossTabulation>(
      std::move(row_queries), std::move(column_queries), std::move(row_filters), std::move(column_filters), std::move(distinct.filters)
   );
}

template <typename SymbolType>
std::unique_ptr<Action> parseConsensus(const json::Value& json) {
   using ConsensusAction = Consensus<SymbolType>;
   const std::string action_name = ConsensusAction::actionName();
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", action_name);
   CHECK_SILO_QUERY(
      (std::is_same_v<SymbolType, Nucleotide>) || sequence_name.has_value(), action_name + " action must contain the field sequenceName of type string (a gene)"
   )
   std::vector<typename ConsensusAction::Group> groups;
   if (json.contains("groups")) {
      CHECK_SILO_QUERY(json["groups"].is_array(), action_name + " action: the field groups, if present, must be an array of objects " + GROUP_ENTRY_FORM)
      const size_t n_groups = json["groups"].items().size();
      CHECK_SILO_QUERY(
         n_groups <= ConsensusAction::MAX_GROUPS,
         action_name + " action: the field groups holds " + std::to_string(n_groups) + " groups, more than the limit of " + std::to_string(ConsensusAction::MAX_GROUPS)
      )
      CHECK_SILO_QUERY(n_groups >= 1, action_name + " action: the field groups, if present, must hold at least one group")
      for (auto& [group_name, filter] : parseGroupEntries(json["groups"], action_name)) {
         groups.push_back({std::move(group_name), std::move(filter)});
      }
   } else {
      groups.push_back({std::nullopt, nullptr});  // the query's filter alone
   }
   double threshold = ConsensusAction::DEFAULT_THRESHOLD;
   if (json.contains("threshold")) {
      CHECK_SILO_QUERY(
         json["threshold"].is_number() && json["threshold"].as_double() > 0 && json["threshold"].as_double() <= 1,
         action_name + " action: the field threshold, if present, must be a number in (0, 1]"
      )
      threshold = json["threshold"].as_double();
   }
   const uint32_t min_depth = integerField(json, "minDepth", action_name, false, 1, UINT32_MAX, "an integer from 1 to " + std::to_string(UINT32_MAX))
                                 .value_or(ConsensusAction::DEFAULT_MIN_DEPTH);
   return std::make_unique<ConsensusAction>(std::move(sequence_name), std::move(groups), threshold, min_depth);
}

template std::unique_ptr<Action> parseConsensus<Nucleotide>(const json::Value& json);
template std::unique_ptr<Action> parseConsensus<AminoAcid>(const json::Value& json);

template <typename SymbolType>
std::unique_ptr<Action> parseMutationsComparison(const json::Value& json) {
   using Comparison = MutationsComparison<SymbolType>;
   const std::string action_name = Comparison::actionName();
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", action_name);
   CHECK_SILO_QUERY(
      (std::is_same_v<SymbolType, Nucleotide>) || sequence_name.has_value(), action_name + " action must contain the field sequenceName of type string (a gene)"
   )
   CHECK_SILO_QUERY(
      json.contains("groups") && json["groups"].is_array(), action_name + " action must contain the field groups: an array of objects " + GROUP_ENTRY_FORM
   )
   const size_t n_groups = json["groups"].items().size();
   CHECK_SILO_QUERY(
      n_groups <= Comparison::MAX_GROUPS,
      action_name + " action: the field groups holds " + std::to_string(n_groups) + " groups, more than the limit of " + std::to_string(Comparison::MAX_GROUPS)
   )
   CHECK_SILO_QUERY(
      n_groups >= Comparison::MIN_GROUPS,
      action_name + " action: the field groups holds " + std::to_string(n_groups) + " groups, fewer than the " + std::to_string(Comparison::MIN_GROUPS) +
         " a comparison needs"
   )
   std::vector<typename Comparison::Group> groups;
   for (auto& [group_name, filter] : parseGroupEntries(json["groups"], action_name)) {
      groups.push_back({std::move(group_name), std::move(filter)});
   }
   double min_proportion = Comparison::DEFAULT_MIN_PROPORTION;
   if (json.contains("minProportion")) {
      CHECK_SILO_QUERY(
         json["minProportion"].is_number(), action_name + " action: the field minProportion, if present, must be of type number with limits [0.0, 1.0]"
      )
      min_proportion = json["minProportion"].as_double();
      CHECK_SILO_QUERY(min_proportion >= 0 && min_proportion <= 1, "Invalid proportion: minProportion must be in interval [0.0, 1.0]")
   }
   double min_difference = Comparison::DEFAULT_MIN_DIFFERENCE;
   if (json.contains("minDifference")) {
      CHECK_SILO_QUERY(
         json["minDifference"].is_number() && json["minDifference"].as_double() >= 0 && json["minDifference"].as_double() <= 1,
         action_name + " action: the field minDifference, if present, must be a number in [0, 1]"
      )
      min_difference = json["minDifference"].as_double();
   }
   return std::make_unique<Comparison>(std::move(sequence_name), std::move(groups), min_proportion, min_difference);
}

template std::unique_ptr<Action> parseMutationsComparison<Nucleotide>(const json::Value& json);
template std::unique_ptr<Action> parseMutationsComparison<AminoAcid>(const json::Value& json);

}  // namespace silo::query_engine::actions
