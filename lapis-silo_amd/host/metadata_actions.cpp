// metadata_actions.cpp — the actions that read metadata columns:
//   Aggregated with groupByFields   src/silo/query_engine/actions/aggregated.cpp:100-149
//   Haplotypes                      (not in the reference) the same group-by with the symbols at listed sequence positions as
//                                   further columns (K16)
//   Details                         src/silo/query_engine/actions/details.cpp
//   Insertions                      src/silo/query_engine/actions/insertions.cpp
// and what the actions that return or compare sequences (sequence_actions.cpp, distance_actions.cpp) read of metadata: columnOf.
#include <algorithm>
#include <cstring>
#include <functional>
#include <set>
#include <type_traits>

#include "query_engine.h"

namespace silo::query_engine::actions {

using storage::column::MetadataColumnPartition;

const MetadataColumnPartition& columnOf(const DatabasePartition& partition, const std::string& name) {
   const auto found = partition.columns.metadata_columns.find(name);
   if (found == partition.columns.metadata_columns.end()) {
      throw std::runtime_error("the metadata column '" + name + "' was not loaded into this database");
   }
   return found->second;
}

namespace {

/// Under position-range sharding every rank holds every row (and every metadata column), so row-wise actions simply
/// run on each rank.  A sequence-id shard is one DatabasePartition of the reference (query_engine.cpp:40-49): an action
/// whose rows are rows of the database (Details; Fasta and FastaAligned, sequence_actions.cpp) answers for ITS rows and the front end concatenates
/// the shards' responses — no collective; ordering, offset and limit then hold per shard.  An action
/// that merges rows across partitions (Aggregated with groupByFields, Insertions) would need a gather that is not built.
void requireRowsMergedLocally(const Database& database, const char* what) {
   if (database.shard_world > 1 && !database.shard_by_position) {
      throw std::runtime_error(std::string(what) + " is not supported on a database sharded by sequence id");
   }
}

/// The group-by of id columns that Aggregated (dictionary ids of metadata columns) and Haplotypes (the same, then tuple ids of
/// sequence positions) share: per partition one count of the mixed-radix tuples of its columns under a row bitset, then every
/// tuple that occurs, as its digits, to the caller's sink — which renders and merges them over partitions.
class TupleCounter {
  public:
   /// (the `launch` number the partition was counted under, one digit per column, the rows that hold the tuple)
   using Sink = std::function<void(size_t launch, const std::vector<uint32_t>& digits, uint32_t count)>;
   explicit TupleCounter(Sink sink) : sink(std::move(sink)) {}

   /// Counts the tuples of `ids` (device columns, `cardinalities` values each; the first column most significant) over the rows of
   /// `rows_bits` — nullptr: the filter's own bitset; otherwise a subset of the filter's rows.  A tuple space of up to
   /// DENSE_HISTOGRAM_LIMIT tuples takes the dense histogram (K6): enqueued on queryStream() and fetched in finish().  A larger one
   /// takes the hash table in HBM keyed by the 64-bit tuple id (K6b), which synchronises: its tuples reach the sink before this
   /// returns.  Nothing the count reads may return to the pool before finish() has returned.
   void launch(
      const DatabasePartition& partition, const OperatorResult& filter, const uint64_t* rows_bits, const std::vector<const uint32_t*>& ids,
      const std::vector<uint32_t>& cardinalities, size_t launch_number
   ) {
      const size_t n_columns = ids.size();
      // the dense histogram comes back whole (4 bytes per potential tuple): beyond a million potential tuples the hash
      // table path, which returns only the tuples that occur, moves less data
      static_assert(DENSE_HISTOGRAM_LIMIT <= SILO_GPU_MAX_GROUP_BINS);
      uint64_t n_bins = 1;  // exact up to the limit; past it only known to be past it (never multiplied again: no wrap)
      for (const uint32_t cardinality : cardinalities) {
         n_bins = n_bins > DENSE_HISTOGRAM_LIMIT ? n_bins : n_bins * std::max<uint32_t>(cardinality, 1);
      }
      if (n_columns <= SILO_GPU_MAX_GROUP_COLUMNS && n_bins <= DENSE_HISTOGRAM_LIMIT) {
         Dense& dense = in_flight.emplace_back();
         dense.launch_number = launch_number;
         dense.cardinalities = cardinalities;
         dense.n_bins = static_cast<size_t>(n_bins);
         dense.device_counts = partition.pool.acquire(dense.n_bins * sizeof(uint32_t));
         checkGpu(silo_gpu_memset_async(dense.device_counts.get(), 0, dense.n_bins * sizeof(uint32_t), queryStream()), "silo_gpu_memset_async");
         checkGpu(
            silo_gpu_group_count(
               partition.store, rows_bits != nullptr ? rows_bits : filter.bitset(), ids.data(), cardinalities.data(), static_cast<uint32_t>(n_columns),
               static_cast<uint32_t*>(dense.device_counts.get()), queryStream()
            ),
            "silo_gpu_group_count"
         );
         dense.fetch = HostFetch(dense.device_counts.get(), dense.n_bins * sizeof(uint32_t), queryStream());
         return;
      }
      // a tuple space beyond the dense histogram: hash table in HBM keyed by the 64-bit tuple id (K6b)
      if (n_columns > SILO_GPU_MAX_GROUP_COLUMNS) {
         throw QueryCompilationException("Compilation Error: more than " + std::to_string(SILO_GPU_MAX_GROUP_COLUMNS) + " groupByFields");
      }
      const uint32_t selected = filter.cardinality();  // (an upper bound of the rows of rows_bits: the table gets twice as many slots)
      if (selected == 0) {
         return;
      }
      uint64_t* device_keys = nullptr;
      uint32_t* device_group_counts = nullptr;
      uint32_t n_groups = 0;
      checkGpu(
         silo_gpu_group_count_hashed(
            partition.store, rows_bits != nullptr ? rows_bits : filter.bitset(), ids.data(), cardinalities.data(), static_cast<uint32_t>(n_columns),
            selected, &device_keys, &device_group_counts, &n_groups, queryStream()
         ),
         "silo_gpu_group_count_hashed"
      );
      std::vector<uint64_t> tuple_ids(n_groups);
      std::vector<uint32_t> tuple_counts(n_groups);
      int status = 0;
      if (n_groups != 0) {
         status = silo_gpu_memcpy_d2h(tuple_ids.data(), device_keys, n_groups * sizeof(uint64_t), queryStream());
         if (status == 0) {
            status = silo_gpu_memcpy_d2h(tuple_counts.data(), device_group_counts, n_groups * sizeof(uint32_t), queryStream());
         }
      }
      silo_gpu_free(device_keys);
      silo_gpu_free(device_group_counts);
      checkGpu(status, "silo_gpu_memcpy_d2h");
      std::vector<uint32_t> digits(n_columns);
      for (uint32_t group = 0; group < n_groups; ++group) {
         digitsOf(tuple_ids[group], cardinalities, digits);
         sink(launch_number, digits, tuple_counts[group]);
      }
   }

   /// Waits for the dense histograms, in launch order, and hands their tuples to the sink.
   void finish() {
      for (Dense& dense : in_flight) {
         const auto* counts = static_cast<const uint32_t*>(dense.fetch.wait());
         std::vector<uint32_t> digits(dense.cardinalities.size());
         for (size_t bin = 0; bin < dense.n_bins; ++bin) {
            if (counts[bin] == 0) {
               continue;
            }
            digitsOf(bin, dense.cardinalities, digits);
            sink(dense.launch_number, digits, counts[bin]);
         }
      }
      in_flight.clear();
   }

  private:
   static constexpr uint64_t DENSE_HISTOGRAM_LIMIT = uint64_t{1} << 20;
   struct Dense {
      size_t launch_number = 0;
      std::vector<uint32_t> cardinalities;
      DeviceBuffer device_counts;
      size_t n_bins = 0;
      HostFetch fetch;
   };
   /// The digits of a mixed-radix tuple id, the first column most significant.
   static void digitsOf(uint64_t tuple_id, const std::vector<uint32_t>& cardinalities, std::vector<uint32_t>& digits) {
      for (size_t column = cardinalities.size(); column-- > 0;) {
         digits[column] = static_cast<uint32_t>(tuple_id % cardinalities[column]);
         tuple_id /= cardinalities[column];
      }
   }
   Sink sink;
   std::vector<Dense> in_flight;
};

}  // namespace

bool tupleSpaceFits(const std::vector<uint32_t>& cardinalities) {
   uint64_t tuples = 1;
   for (const uint32_t cardinality : cardinalities) {
      if (__builtin_mul_overflow(tuples, static_cast<uint64_t>(std::max<uint32_t>(cardinality, 1)), &tuples)) {
         return false;
      }
   }
   return tuples < UINT64_MAX;
}

// ---- Aggregated with groupByFields ---------------------------------------------------------------------
QueryResult Aggregated::aggregateWithGrouping(const Database& database, std::vector<OperatorResult>& bitmap_filter) const {
   requireRowsMergedLocally(database, "Aggregated with groupByFields");
   struct Group {
      uint32_t count = 0;
      std::vector<JsonValue> values;
   };
   // Tuples are keyed by their raw bytes (tuple.cpp:389-391); std::map instead of the reference's unordered_map
   // makes the (unspecified) order of the result rows deterministic.
   std::map<std::string, Group> groups;
   const size_t n_fields = group_by_fields.size();

   std::vector<std::vector<const MetadataColumnPartition*>> launched;  // the columns of every counted partition
   std::string key;
   TupleCounter counter([&](size_t launch, const std::vector<uint32_t>& digits, uint32_t count) {
      const std::vector<const MetadataColumnPartition*>& columns = launched[launch];
      key.clear();
      for (size_t field = 0; field < n_fields; ++field) {
         columns[field]->appendKeyOfGroup(digits[field], key);
      }
      Group& group = groups[key];
      if (group.count == 0) {
         for (size_t field = 0; field < n_fields; ++field) {
            group.values.push_back(columns[field]->jsonOfGroup(digits[field]));
         }
      }
      group.count += count;
   });
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      OperatorResult& filter = bitmap_filter[partition_id];
      std::vector<const MetadataColumnPartition*> columns;
      for (const std::string& field : group_by_fields) {
         columns.push_back(&columnOf(partition, field));
      }
      if (partition.sequence_count == 0) {
         continue;
      }
      // dictionary ids per field: a tuple is a mixed-radix number, the histogram of those numbers is the group-by
      std::vector<const uint32_t*> ids;
      std::vector<uint32_t> cardinalities;
      for (const MetadataColumnPartition* column : columns) {
         const MetadataColumnPartition::Groups column_groups = column->groups();
         ids.push_back(column_groups.device_ids);
         cardinalities.push_back(column_groups.cardinality);
      }
      launched.push_back(std::move(columns));
      counter.launch(partition, filter, nullptr, ids, cardinalities, launched.size() - 1);
   }
   Trace::mark("groups_launched");
   counter.finish();
   Trace::mark("groups_on_host");
   QueryResult result;  // generateResult, aggregated.cpp:44-56
   result.query_result.reserve(groups.size());
   for (auto& [key, group] : groups) {
      QueryResultEntry& entry = result.query_result.emplace_back();
      for (size_t field = 0; field < n_fields; ++field) {
         entry.fields[group_by_fields[field]] = std::move(group.values[field]);
      }
      entry.fields["count"] = static_cast<int32_t>(group.count);
   }
   return result;
}

// ---- Haplotypes / AminoAcidHaplotypes --------------------------------------------------------------------
// The combinations of symbols at listed positions and their counts: the group-by above with the symbol columns of K16 behind the
// metadata columns, with its parser.  No counterpart in the reference.
template <typename SymbolType>
void Haplotypes<SymbolType>::validateOrderByFields(const Database& database) const {
   const std::string action_name = actionName();
   for (const std::string& group_by_field : group_by_fields) {  // resolved as Aggregated resolves them
      CHECK_SILO_QUERY(
         database.database_config.getMetadata(group_by_field).has_value(),
         action_name + " action: the metadata field '" + group_by_field + "' of groupByFields to group by was not found"
      )
   }
   for (const OrderByField& field : order_by_fields) {
      CHECK_SILO_QUERY(
         field.name == "haplotype" || field.name == "count" || field.name == "proportion" ||
            std::find(group_by_fields.begin(), group_by_fields.end(), field.name) != group_by_fields.end(),
         "The orderByField '" + field.name + "' cannot be ordered by, as it is neither haplotype, count, proportion nor one of the groupByFields."
      )
   }
}

template <typename SymbolType>
QueryResult Haplotypes<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = actionName();
   requireUnsharded(database, action_name);
   const auto [name, store] = sequenceStoreOf<SymbolType>(
      database, sequence_name, action_name + " action: the database does not contain the " + std::string(SymbolType::SYMBOL_NAME_LOWER_CASE) + " sequence with name: "
   );
   const size_t length = store.reference_sequence.size();
   const auto n_positions = static_cast<uint32_t>(positions.size());
   std::vector<uint32_t> listed;  // 0-based
   for (const uint32_t position : positions) {
      CHECK_SILO_QUERY(
         position >= 1 && position <= length,
         action_name + " action: the position " + std::to_string(position) + " of the field positions is outside the sequence '" + name + "' (1 to " +
            std::to_string(length) + ")"
      )
      listed.push_back(position - 1);
   }
   constexpr uint32_t n_symbols = SymbolType::COUNT;
   static_assert(n_symbols <= 32);
   uint32_t complete_symbols = UINT32_MAX;
   if (exclude_incomplete) {
      complete_symbols = 0;
      for (const auto symbol : SymbolType::VALID_MUTATION_SYMBOLS) {
         complete_symbols |= 1u << static_cast<uint32_t>(symbol);
      }
   }
   // the id columns of the positions, POSITIONS_PER_COLUMN to a column, and the tuple space of each
   const size_t n_fields = group_by_fields.size();
   const uint32_t n_id_columns = (n_positions + POSITIONS_PER_COLUMN - 1) / POSITIONS_PER_COLUMN;
   std::vector<uint32_t> id_positions(n_id_columns), id_cardinalities(n_id_columns, 1);
   for (uint32_t j = 0; j < n_id_columns; ++j) {
      id_positions[j] = std::min(POSITIONS_PER_COLUMN, n_positions - j * POSITIONS_PER_COLUMN);
      for (uint32_t i = 0; i < id_positions[j]; ++i) {
         id_cardinalities[j] *= n_symbols;
      }
   }

   // what every partition with selected rows is counted over, checked before anything is launched
   struct Counted {
      const DatabasePartition* partition;
      OperatorResult* filter;
      std::vector<const MetadataColumnPartition*> columns;
      std::vector<const uint32_t*> ids;
      std::vector<uint32_t> cardinalities;
      uint32_t seqstore_id;
      DeviceBuffer scratch;  // the symbol columns, the id columns, the bitset of the complete rows, the unresolved word
      HostFetch unresolved;
   };
   std::vector<Counted> counted;
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      std::vector<const MetadataColumnPartition*> columns;
      for (const std::string& field : group_by_fields) {
         columns.push_back(&columnOf(partition, field));
      }
      if (partition.sequence_count == 0 || bitmap_filter[partition_id].cardinality() == 0) {
         continue;
      }
      Counted& entry = counted.emplace_back();
      entry.partition = &partition;
      entry.filter = &bitmap_filter[partition_id];
      entry.seqstore_id = partition.getSequenceStores<SymbolType>().at(name).seqstore_id;
      for (const MetadataColumnPartition* column : columns) {
         const MetadataColumnPartition::Groups column_groups = column->groups();
         entry.ids.push_back(column_groups.device_ids);
         entry.cardinalities.push_back(column_groups.cardinality);
      }
      entry.columns = std::move(columns);
      entry.cardinalities.insert(entry.cardinalities.end(), id_cardinalities.begin(), id_cardinalities.end());
      CHECK_SILO_QUERY(
         tupleSpaceFits(entry.cardinalities),
         action_name + " action: the tuple space of the groupByFields and the " + std::to_string(n_positions) +
            " positions holds 2^64 - 1 combinations or more; list fewer positions or fewer groupByFields"
      )
   }

   struct Group {
      uint64_t count = 0;
      std::vector<JsonValue> values;
      std::string haplotype;
   };
   std::map<std::string, Group> groups;  // keyed as Aggregated keys its tuples, the haplotype's characters last
   std::string key, haplotype;
   TupleCounter counter([&](size_t launch, const std::vector<uint32_t>& digits, uint32_t count) {
      const std::vector<const MetadataColumnPartition*>& columns = counted[launch].columns;
      key.clear();
      for (size_t field = 0; field < n_fields; ++field) {
         columns[field]->appendKeyOfGroup(digits[field], key);
      }
      haplotype.assign(n_positions, '?');
      for (uint32_t j = 0; j < n_id_columns; ++j) {
         uint32_t rest = digits[n_fields + j];  // the column's first position most significant
         for (uint32_t i = id_positions[j]; i-- > 0;) {
            haplotype[j * POSITIONS_PER_COLUMN + i] = SymbolType::symbolToChar(static_cast<typename SymbolType::Symbol>(rest % n_symbols));
            rest /= n_symbols;
         }
      }
      key += haplotype;
      Group& group = groups[key];
      if (group.count == 0) {
         for (size_t field = 0; field < n_fields; ++field) {
            group.values.push_back(columns[field]->jsonOfGroup(digits[field]));
         }
         group.haplotype = haplotype;
      }
      group.count += count;
   });
   launchAndWait([&] {  // (nothing in `counted` returns to the pool before: the launches read and write it)
      for (size_t launch = 0; launch < counted.size(); ++launch) {
         Counted& entry = counted[launch];
         const DatabasePartition& partition = *entry.partition;
         const uint32_t row_words = partition.rowWords();
         const size_t rows = static_cast<size_t>(row_words) * 64;
         const size_t symbol_bytes = n_positions * rows;
         const size_t id_bytes = n_id_columns * rows * sizeof(uint32_t);
         const size_t bitset_bytes = static_cast<size_t>(row_words) * sizeof(uint64_t);
         entry.scratch = partition.pool.acquire(symbol_bytes + id_bytes + bitset_bytes + sizeof(uint64_t));
         auto* device_symbols = entry.scratch.template as<uint8_t>();
         auto* device_ids = reinterpret_cast<uint32_t*>(device_symbols + symbol_bytes);
         auto* device_rows = reinterpret_cast<uint64_t*>(device_symbols + symbol_bytes + id_bytes);
         auto* device_unresolved = reinterpret_cast<uint32_t*>(device_symbols + symbol_bytes + id_bytes + bitset_bytes);
         checkGpu(
            silo_gpu_position_symbols(partition.store, entry.seqstore_id, listed.data(), n_positions, device_symbols, device_unresolved, queryStream()),
            "silo_gpu_position_symbols"
         );
         entry.unresolved = HostFetch(device_unresolved, sizeof(uint32_t), queryStream());
         uint32_t* id_columns[MAX_ID_COLUMNS] = {};
         for (uint32_t j = 0; j < n_id_columns; ++j) {
            id_columns[j] = device_ids + j * rows;
            entry.ids.push_back(id_columns[j]);
         }
         // the rows that are counted: the filter's, or with excludeIncomplete those of them whose listed symbols are all valid
         const uint64_t* filter_bits = entry.filter->bitset();
         checkGpu(
            silo_gpu_haplotype_ids(
               device_symbols, n_positions, row_words, partition.sequence_count, n_symbols, complete_symbols, filter_bits, id_columns,
               exclude_incomplete ? device_rows : nullptr, queryStream()
            ),
            "silo_gpu_haplotype_ids"
         );
         counter.launch(partition, *entry.filter, exclude_incomplete ? device_rows : filter_bits, entry.ids, entry.cardinalities, launch);
      }
      Trace::mark("haplotypes_launched");
      for (const Counted& entry : counted) {
         uint32_t unresolved = 0;
         std::memcpy(&unresolved, entry.unresolved.wait(), sizeof(unresolved));
         if (unresolved != 0) {
            throw std::runtime_error(
               action_name + ": the sequence store '" + name + "' holds " + std::to_string(unresolved) +
               " cells at the listed positions that no stored symbol claims"
            );
         }
      }
      counter.finish();
   });
   Trace::mark("haplotypes_on_host");

   uint64_t total = 0;
   for (const auto& [tuple_key, group] : groups) {
      total += group.count;
   }
   QueryResult result;
   result.query_result.reserve(groups.size());
   for (auto& [tuple_key, group] : groups) {
      QueryResultEntry& entry = result.query_result.emplace_back();
      for (size_t field = 0; field < n_fields; ++field) {
         entry.fields[group_by_fields[field]] = std::move(group.values[field]);
      }
      entry.fields["haplotype"] = std::move(group.haplotype);
      entry.fields["count"] = static_cast<int32_t>(group.count);
      entry.fields["proportion"] = static_cast<double>(group.count) / static_cast<double>(total);  // (a row exists: total >= 1)
   }
   return result;
}

template class Haplotypes<Nucleotide>;
template class Haplotypes<AminoAcid>;

template <typename SymbolType>
std::unique_ptr<Action> parseHaplotypes(const json::Value& json) {
   using HaplotypesAction = Haplotypes<SymbolType>;
   const std::string action_name = HaplotypesAction::actionName();
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", action_name);
   CHECK_SILO_QUERY(
      (std::is_same_v<SymbolType, Nucleotide>) || sequence_name.has_value(), action_name + " action must contain the field sequenceName of type string (a gene)"
   )
   const std::string positions_form =
      action_name + " action: the field positions must be an array of 1 to " + std::to_string(HaplotypesAction::MAX_POSITIONS) + " distinct positions (integers from 1)";
   CHECK_SILO_QUERY(json.contains("positions") && json["positions"].is_array() && !json["positions"].items().empty(), positions_form)
   const size_t n_positions = json["positions"].items().size();
   CHECK_SILO_QUERY(
      n_positions <= HaplotypesAction::MAX_POSITIONS, positions_form + "; it holds " + std::to_string(n_positions)
   )
   std::vector<uint32_t> positions;
   std::set<uint32_t> seen;
   for (const auto& element : json["positions"].items()) {
      CHECK_SILO_QUERY(
         element.is_number_unsigned() && element.as_int64() >= 1 && element.as_int64() <= UINT32_MAX,
         positions_form + "; found the element " + element.dump()
      )
      const uint32_t position = element.as_uint32();
      CHECK_SILO_QUERY(seen.insert(position).second, positions_form + "; the position " + std::to_string(position) + " occurs more than once")
      positions.push_back(position);
   }
   std::vector<std::string> group_by_fields;
   if (json.contains("groupByFields")) {
      const std::string fields_form = action_name + " action: the field groupByFields, if present, must be an array of at most " +
                                      std::to_string(HaplotypesAction::MAX_FIELDS) + " metadata field names (strings)";
      CHECK_SILO_QUERY(json["groupByFields"].is_array(), fields_form)
      CHECK_SILO_QUERY(
         json["groupByFields"].items().size() <= HaplotypesAction::MAX_FIELDS, fields_form + "; it holds " + std::to_string(json["groupByFields"].items().size())
      )
      for (const auto& element : json["groupByFields"].items()) {
         CHECK_SILO_QUERY(element.is_string(), fields_form + "; found the element " + element.dump())
         group_by_fields.push_back(element.as_string());
      }
   }
   bool exclude_incomplete = false;
   if (json.contains("excludeIncomplete")) {
      CHECK_SILO_QUERY(json["excludeIncomplete"].is_boolean(), action_name + " action: the field excludeIncomplete, if present, must be of type boolean")
      exclude_incomplete = json["excludeIncomplete"].as_bool();
   }
   return std::make_unique<HaplotypesAction>(std::move(sequence_name), std::move(positions), std::move(group_by_fields), exclude_incomplete);
}

template std::unique_ptr<Action> parseHaplotypes<Nucleotide>(const json::Value& json);
template std::unique_ptr<Action> parseHaplotypes<AminoAcid>(const json::Value& json);

// ---- Details ---------------------------------------------------------------------------------------------
namespace {

std::vector<storage::ColumnMetadata> parseFields(const Database& database, const std::vector<std::string>& fields) {  // details.cpp:22-35
   if (fields.empty()) {
      return database.database_config.metadata;
   }
   std::vector<storage::ColumnMetadata> field_metadata;
   for (const std::string& field : fields) {
      const auto metadata = database.database_config.getMetadata(field);
      CHECK_SILO_QUERY(metadata.has_value(), "Metadata field " + field + " not found.")
      field_metadata.push_back(*metadata);
   }
   return field_metadata;
}

}  // namespace

void Details::validateOrderByFields(const Database& database) const {  // details.cpp:43-59
   const std::vector<storage::ColumnMetadata> field_metadata = parseFields(database, fields);
   for (const OrderByField& field : order_by_fields) {
      CHECK_SILO_QUERY(
         std::any_of(field_metadata.begin(), field_metadata.end(), [&](const storage::ColumnMetadata& metadata) { return metadata.name == field.name; }),
         "OrderByField " + field.name + " is not contained in the result of this operation."
      )
   }
}

QueryResult Details::execute(const Database& /*database*/, std::vector<OperatorResult> /*bitmap_filter*/) const {
   return QueryResult{};  // details.cpp:61-66: everything happens in executeAndOrder
}

QueryResult Details::finish(const Database& database, Pending& pending) const {
   return executeAndOrder(database, std::move(pending.bitmap_filter));
}

QueryResult Details::executeAndOrder(const Database& database, std::vector<OperatorResult> bitmap_filter) const {  // details.cpp:186-219
   validateOrderByFields(database);
   const std::vector<storage::ColumnMetadata> field_metadata = parseFields(database, fields);

   struct Row {
      uint32_t partition;
      uint32_t row;
   };
   std::vector<Row> tuples;
   // columns of every partition, in field order (the TupleFactory of a partition)
   std::vector<std::vector<const storage::column::MetadataColumnPartition*>> columns(database.partitions.size());
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      for (const auto& metadata : field_metadata) {
         columns[partition_id].push_back(&columnOf(partition, metadata.name));
      }
      for (const uint32_t row : selectedRows(partition, bitmap_filter[partition_id])) {
         tuples.push_back({static_cast<uint32_t>(partition_id), row});
      }
   }
   Trace::mark("rows_selected");

   // Tuple::compareLess (tuple.cpp:372-387) over the orderByFields, on the raw column values
   struct CompareField {
      size_t index;
      bool ascending;
   };
   std::vector<CompareField> compare_fields;
   for (const OrderByField& order_by : order_by_fields) {
      for (size_t index = 0; index < field_metadata.size(); ++index) {
         if (field_metadata[index].name == order_by.name) {
            compare_fields.push_back({index, order_by.ascending});
            break;
         }
      }
   }
   const auto less = [&](const Row& a, const Row& b) {
      for (const CompareField& field : compare_fields) {
         const int compared = columns[a.partition][field.index]->compareRows(a.row, *columns[b.partition][field.index], b.row);
         if (compared < 0) {
            return field.ascending;
         }
         if (compared > 0) {
            return !field.ascending;
         }
      }
      return false;
   };
   // With a limit the reference keeps the `limit + offset` smallest tuples per partition in a heap and merges
   // them (:88-147).  Its heap is offered the first row past the prefix twice (:118-134), which can duplicate a
   // row in the result; that defect is not reproduced: the smallest `limit + offset` tuples, each once.
   size_t to_produce = tuples.size();
   if (limit.has_value()) {
      to_produce = std::min<size_t>(tuples.size(), static_cast<size_t>(limit.value()) + offset.value_or(0));
   }
   if (!compare_fields.empty()) {
      if (to_produce < tuples.size()) {
         std::partial_sort(tuples.begin(), tuples.begin() + static_cast<int64_t>(to_produce), tuples.end(), less);
      } else {
         std::sort(tuples.begin(), tuples.end(), less);
      }
   }
   tuples.resize(to_produce);

   // only the rows that survive offset / limit are rendered (applyOffsetAndLimit, action.cpp:68-91)
   const size_t begin = std::min<size_t>(offset.value_or(0), tuples.size());
   QueryResult results_in_format;
   results_in_format.query_result.reserve(tuples.size() - begin);
   for (size_t index = begin; index < tuples.size(); ++index) {
      const Row& tuple = tuples[index];
      QueryResultEntry& entry = results_in_format.query_result.emplace_back();
      for (size_t field = 0; field < field_metadata.size(); ++field) {
         entry.fields[field_metadata[field].name] = columns[tuple.partition][field]->jsonOfRow(tuple.row);
      }
   }
   Trace::mark("rows_built");
   return results_in_format;
}

// ---- Insertions / AminoAcidInsertions (insertions.cpp) ---------------------------------------------------
template <typename SymbolType>
void InsertionAggregation<SymbolType>::validateOrderByFields(const Database& /*database*/) const {  // :41-59
   checkOrderByFields({"position", "insertions", "sequenceName", "count"});
}

template <typename SymbolType>
QueryResult InsertionAggregation<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {  // :126-258
   const config::ColumnType wanted_type =
      std::is_same_v<SymbolType, Nucleotide> ? config::ColumnType::NUC_INSERTION : config::ColumnType::AA_INSERTION;
   for (const std::string& column_name : column_names) {  // validateDatabaseColumnNames
      const auto metadata = database.database_config.getMetadata(column_name);
      CHECK_SILO_QUERY(
         metadata.has_value() && metadata->type == wanted_type,
         "The database does not contain the " + std::string(SymbolType::SYMBOL_NAME) + " column '" + column_name + "'"
      )
   }
   for (const std::string& sequence_name : sequence_names) {  // validateSequenceNames
      CHECK_SILO_QUERY(
         database.getSequenceStores<SymbolType>().count(sequence_name) != 0,
         "The database does not contain the " + std::string(SymbolType::SYMBOL_NAME) + " sequence '" + sequence_name + "'"
      )
   }
   requireRowsMergedLocally(database, "Insertions");

   // One k_count_pairs launch per (partition, column, sequence): the and_cardinality of the filter with the rows of
   // every distinct insertion at once (:196-206).  Launch all, then fetch.
   struct InFlight {
      const std::string* sequence_name;
      const storage::column::InsertionColumnPartition::SequenceIndex* index;
      DeviceBuffer device_counts;
      HostFetch fetch;
   };
   std::vector<InFlight> in_flight;
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      const auto& insertion_columns = partition.columns.getInsertionColumns<SymbolType>();
      for (const std::string& column_name : column_names) {  // validatePartitionColumnNames
         CHECK_SILO_QUERY(
            insertion_columns.count(column_name) != 0,
            "The database does not contain the " + std::string(SymbolType::SYMBOL_NAME) + " column '" + column_name + "'"
         )
      }
      OperatorResult& filter = bitmap_filter[partition_id];
      if (filter.cardinality() == 0) {
         continue;
      }
      for (const auto& [column_name, insertion_column] : insertion_columns) {
         if (!column_names.empty() && std::find(column_names.begin(), column_names.end(), column_name) == column_names.end()) {
            continue;
         }
         for (const auto& [sequence_name, index] : insertion_column.getInsertionIndexes()) {
            if (!sequence_names.empty() && std::find(sequence_names.begin(), sequence_names.end(), sequence_name) == sequence_names.end()) {
               continue;
            }
            if (index.insertions.empty()) {
               continue;
            }
            InFlight& launch = in_flight.emplace_back();
            launch.sequence_name = &sequence_name;
            launch.index = &index;
            const size_t bytes = index.insertions.size() * sizeof(uint32_t);
            launch.device_counts = partition.pool.acquire(bytes);
            checkGpu(silo_gpu_memset_async(launch.device_counts.get(), 0, bytes, queryStream()), "silo_gpu_memset_async");
            checkGpu(
               silo_gpu_count_pairs(
                  partition.store, filter.bitset(), index.device_rows, index.device_ids, static_cast<uint32_t>(index.pair_rows.size()),
                  static_cast<uint32_t*>(launch.device_counts.get()), queryStream()
               ),
               "silo_gpu_count_pairs"
            );
            launch.fetch = HostFetch(launch.device_counts.get(), bytes, queryStream());
         }
      }
   }
   // sequence name -> (position, insertion) -> count; the reference's unordered_maps leave the row order unspecified
   std::map<std::string, std::map<std::pair<uint32_t, std::string>, uint32_t>> all_insertions;
   for (const InFlight& launch : in_flight) {
      const auto* counts = static_cast<const uint32_t*>(launch.fetch.wait());
      auto& per_sequence = all_insertions[*launch.sequence_name];
      for (size_t id = 0; id < launch.index->insertions.size(); ++id) {
         if (counts[id] > 0) {
            per_sequence[{launch.index->positions[id], launch.index->insertions[id]}] += counts[id];
         }
      }
   }
   QueryResult result;
   for (const auto& [sequence_name, per_sequence] : all_insertions) {
      for (const auto& [position_and_insertion, count] : per_sequence) {
         QueryResultEntry& entry = result.query_result.emplace_back();
         entry.fields["position"] = static_cast<int32_t>(position_and_insertion.first);
         entry.fields["sequenceName"] = sequence_name;
         entry.fields["insertions"] = position_and_insertion.second;
         entry.fields["count"] = static_cast<int32_t>(count);
      }
   }
   return result;
}

template class InsertionAggregation<Nucleotide>;
template class InsertionAggregation<AminoAcid>;

}  // namespace silo::query_engine::actions
