// sequence_actions.cpp — the actions whose rows are sequences of the selected rows, with their parser:
//   Fasta                   src/silo/query_engine/actions/fasta.cpp
//   FastaAligned            src/silo/query_engine/actions/fasta_aligned.cpp
//   MutationsPerSequence    (not in the reference) FastaAligned's rows as each row's differences from the reference (K18)
//   CellCountDistribution   (not in the reference) the histogram of the selected rows' cell counts (K22)
//   CellCountByRegion       (not in the reference) per region of positions, the selected rows whose cell count there is in bounds (K23)
// and what every action that reads the selected rows' sequences begins with, the distance actions (distance_actions.cpp) among
// them: selectedRows, selectedCount, the description of an aligned sequence by name (alignedSequence), and the one walk over the
// selection that uploads a partition's row ids and hands them to the caller's gather (SelectedSequences).
#include <algorithm>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "query_engine.h"

namespace silo::query_engine::actions {

using storage::column::MetadataColumnPartition;

/// The set bits of a filter, fetched from the device.
std::vector<uint32_t> selectedRows(const DatabasePartition& partition, const OperatorResult& filter) {
   std::vector<uint32_t> rows;
   const uint32_t cardinality = filter.cardinality();
   if (cardinality == 0) {
      return rows;
   }
   rows.reserve(cardinality);
   std::vector<uint64_t> words(partition.rowWords());
   checkGpu(silo_gpu_memcpy_d2h(words.data(), filter.bitset(), words.size() * sizeof(uint64_t), queryStream()), "silo_gpu_memcpy_d2h");
   for (size_t word = 0; word < words.size(); ++word) {
      uint64_t bits = words[word];
      while (bits != 0) {
         rows.push_back(static_cast<uint32_t>(word * 64 + static_cast<uint32_t>(__builtin_ctzll(bits))));
         bits &= bits - 1;
      }
   }
   return rows;
}

size_t selectedCount(const Database& database, const std::vector<OperatorResult>& bitmap_filter) {
   size_t total_count = 0;
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      total_count += database.partitions[partition_id].sequence_count == 0 ? 0 : bitmap_filter[partition_id].cardinality();
   }
   return total_count;
}

AlignedSequence alignedSequence(const Database& database, const std::optional<std::string>& sequence_name, const std::string& complaint) {
   AlignedSequence sequence;
   sequence.name = sequence_name.value_or(database.database_config.default_nucleotide_sequence);
   const auto nucleotide = database.nuc_sequences.find(sequence.name);
   const auto amino_acid = database.aa_sequences.find(sequence.name);
   sequence.is_amino_acid = nucleotide == database.nuc_sequences.end();
   CHECK_SILO_QUERY(!sequence.is_amino_acid || amino_acid != database.aa_sequences.end(), complaint + "'" + sequence.name + "'")
   sequence.alphabet = sequence.is_amino_acid ? SILO_GPU_ALPHABET_AMINO_ACID : SILO_GPU_ALPHABET_NUCLEOTIDE;
   sequence.positions =
      static_cast<uint32_t>(sequence.is_amino_acid ? amino_acid->second.reference_sequence.size() : nucleotide->second.reference_sequence.size());
   return sequence;
}

uint32_t AlignedSequence::seqstoreOf(const DatabasePartition& partition) const {
   return is_amino_acid ? partition.aa_sequences.at(name).seqstore_id : partition.nuc_sequences.at(name).seqstore_id;
}

void SelectedSequences::gather(
   const Database& database, const std::vector<OperatorResult>& bitmap_filter, size_t n, const std::string& what, bool numbered, const Step& step
) {
   const std::string& primary_key_column = database.database_config.primary_key;
   keys.reserve(n);
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      if (partition.sequence_count == 0) {
         continue;
      }
      const std::vector<uint32_t> rows = selectedRows(partition, bitmap_filter[partition_id]);
      if (rows.empty()) {
         continue;
      }
      const size_t first_sequence = keys.size();
      if (first_sequence + rows.size() > n) {
         throw std::runtime_error(what + ": a filter selects more rows than its cardinality says");
      }
      const MetadataColumnPartition& primary_key = columnOf(partition, primary_key_column);
      for (const uint32_t row : rows) {
         keys.push_back(primary_key.jsonOfRow(row));
         if (numbered) {
            numbering.emplace_back(static_cast<uint32_t>(partition_id), row);
         }
      }
      if (!step) {
         continue;
      }
      auto* device_rows = row_ids.emplace_back(partition.pool.acquire(rows.size() * sizeof(uint32_t))).as<uint32_t>();
      checkGpu(silo_gpu_memcpy_h2d(device_rows, rows.data(), rows.size() * sizeof(uint32_t), queryStream()), "silo_gpu_memcpy_h2d");
      step(partition, device_rows, static_cast<uint32_t>(rows.size()), first_sequence);
   }
   if (keys.size() != n) {
      throw std::runtime_error(what + ": a filter selects fewer rows than its cardinality says");
   }
}

namespace {

/// Needs every position of a sequence on this device: not on a position-range shard.  (A sequence-id shard answers for ITS rows and
/// the front end concatenates the shards' responses: see requireRowsMergedLocally, metadata_actions.cpp.)
void requireAllPositionsLocal(const Database& database, const char* what) {
   if (database.shard_world > 1 && database.shard_by_position) {
      throw std::runtime_error(std::string(what) + " is not supported on a database sharded by position range");
   }
}

/// validateOrderByFields of Fasta (fasta.cpp:42-57) and FastaAligned (fasta_aligned.cpp:28-42): the primary key or a requested sequence.
void checkSequenceOrderByFields(
   const Database& database, const std::vector<OrderByField>& order_by_fields, const std::vector<std::string>& sequence_names, const char* action_name
) {
   const std::string& primary_key_field = database.database_config.primary_key;
   for (const OrderByField& field : order_by_fields) {
      std::string joined;
      for (size_t i = 0; i < sequence_names.size(); ++i) {
         joined += (i == 0 ? "" : ",") + sequence_names[i];
      }
      CHECK_SILO_QUERY(
         field.name == primary_key_field || std::find(sequence_names.begin(), sequence_names.end(), field.name) != sequence_names.end(),
         "The only fields returned by the " + std::string(action_name) + " action are " + joined + " and " + primary_key_field
      )
   }
}

}  // namespace

// ---- Fasta (fasta.cpp) ---------------------------------------------------------------------------------------
void Fasta::validateOrderByFields(const Database& database) const {
   checkSequenceOrderByFields(database, order_by_fields, sequence_names, "Fasta");
}

QueryResult Fasta::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {  // :214-245
   for (const std::string& sequence_name : sequence_names) {
      // every nucleotide sequence has an unaligned store (database.cpp:664-673)
      CHECK_SILO_QUERY(
         database.nuc_sequences.count(sequence_name) != 0, "Database does not contain an unaligned sequence with name: '" + sequence_name + "'"
      )
   }
   const std::string& primary_key_column = database.database_config.primary_key;
   const size_t total_count = selectedCount(database, bitmap_filter);
   CHECK_SILO_QUERY(total_count <= SEQUENCE_LIMIT, "Fasta action currently limited to " + std::to_string(SEQUENCE_LIMIT) + " sequences")
   QueryResult results;
   results.query_result.reserve(total_count);
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      const std::vector<uint32_t> rows = selectedRows(partition, bitmap_filter[partition_id]);
      if (rows.empty()) {
         continue;
      }
      const MetadataColumnPartition& primary_key = columnOf(partition, primary_key_column);
      for (const uint32_t row : rows) {
         QueryResultEntry& entry = results.query_result.emplace_back();
         JsonValue key = primary_key.jsonOfRow(row);
         if (!key.has_value()) {
            throw std::runtime_error("Detected primary_key in column '" + primary_key_column + "' that is null.");
         }
         entry.fields.emplace(primary_key_column, std::move(key));
         for (const std::string& sequence_name : sequence_names) {
            const auto found = partition.unaligned_nuc_sequences.find(sequence_name);
            if (found != partition.unaligned_nuc_sequences.end() && row < found->second.size() && found->second[row].has_value()) {
               entry.fields.emplace(sequence_name, *found->second[row]);
            } else {
               entry.fields.emplace(sequence_name, std::nullopt);
            }
         }
      }
   }
   return results;
}

// ---- FastaAligned (fasta_aligned.cpp) ----------------------------------------------------------------------
void FastaAligned::validateOrderByFields(const Database& database) const {
   checkSequenceOrderByFields(database, order_by_fields, sequence_names, "FastaAligned");
}

QueryResult FastaAligned::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {  // :85-136
   std::vector<AlignedSequence> requested;  // nucleotide sequences first, then genes (:89-103); the row is a map anyway
   for (const std::string& sequence_name : sequence_names) {
      requested.push_back(alignedSequence(database, sequence_name, "Database does not contain a sequence with name: "));
   }
   const size_t total_count = selectedCount(database, bitmap_filter);
   CHECK_SILO_QUERY(total_count < 10001, "FastaAligned action currently limited to 10000 sequences")
   requireAllPositionsLocal(database, "FastaAligned");

   const std::string& primary_key_column = database.database_config.primary_key;
   QueryResult results;
   results.query_result.resize(total_count);
   SelectedSequences selection;  // owns the row ids that the gathers read; every gather ends in a synchronous copy
   waitIfThrown([&] {
      selection.gather(
         database, bitmap_filter, total_count, "FastaAligned", false,
         [&](const DatabasePartition& partition, const uint32_t* device_rows, uint32_t n_rows, size_t first_sequence) {
            for (size_t index = 0; index < n_rows; ++index) {
               results.query_result[first_sequence + index].fields.emplace(primary_key_column, std::move(selection.keys[first_sequence + index]));
            }
            // reconstructSequence (:44-83) for all selected rows of a store at once: one gather over the planes
            for (const AlignedSequence& sequence : requested) {
               const size_t length = sequence.positions;
               std::vector<char> chars(n_rows * length);
               if (!chars.empty()) {
                  const DeviceBuffer device_chars = partition.pool.acquire(chars.size());
                  checkGpu(
                     silo_gpu_reconstruct_sequences(partition.store, sequence.seqstoreOf(partition), device_rows, n_rows, device_chars.as<char>(), queryStream()),
                     "silo_gpu_reconstruct_sequences"
                  );
                  checkGpu(silo_gpu_memcpy_d2h(chars.data(), device_chars.get(), chars.size(), queryStream()), "silo_gpu_memcpy_d2h");
               }
               for (size_t index = 0; index < n_rows; ++index) {
                  results.query_result[first_sequence + index].fields.emplace(sequence.name, std::string(chars.data() + index * length, length));
               }
            }
         }
      );
   });
   return results;
}

// ---- MutationsPerSequence / AminoAcidMutationsPerSequence -------------------------------------------------
// Each selected sequence's differences from the reference, from the rows FastaAligned would return, on the device (K18).  No
// counterpart in the reference.
namespace {

/// The class of a cell as silo_gpu_sequence_differences defines it (include/silo_gpu.h), on the host's reference.
enum class CellClass : uint8_t { SAME, SUBSTITUTION, DELETION, MISSING, AMBIGUOUS };

template <typename SymbolType>
CellClass classOfCell(uint8_t byte, char reference) {
   const auto character = static_cast<char>(byte);
   if (character == SymbolType::symbolToChar(SymbolType::SYMBOL_MISSING)) {
      return CellClass::MISSING;
   }
   bool valid = false;
   for (const auto symbol : SymbolType::VALID_MUTATION_SYMBOLS) {
      valid = valid || SymbolType::symbolToChar(symbol) == character;
   }
   if (!valid) {
      return CellClass::AMBIGUOUS;
   }
   if (character == reference) {
      return CellClass::SAME;
   }
   return character == '-' ? CellClass::DELETION : CellClass::SUBSTITUTION;
}

/// What one row's record words say, as the response's four lists and four counts.
struct RowDifferences {
   std::string lists[SILO_GPU_DIFFERENCE_STATS];   // substitutions, deletions, missing, ambiguous
   uint32_t cells[SILO_GPU_DIFFERENCE_STATS] = {};  // the cells behind each
};

/// Reads the words [begin, end) of one row and checks them on the way: positions strictly ascending and inside the sequence, a
/// close only directly after a run start, every byte a symbol of the alphabet whose class against `reference` is the one its record
/// kind needs, no run start that continues a run of its own class.  A run ends where the next record stands, or with the sequence.
/// An empty string: the row is sound.
template <typename SymbolType>
std::string readRowDifferences(const uint32_t* begin, const uint32_t* end, const std::string& reference, RowDifferences& row) {
   const auto positions = static_cast<uint32_t>(reference.size());
   const auto append = [](std::string& list, const std::string& item) {
      list += list.empty() ? "" : ",";
      list += item;
   };
   bool run_open = false;          // a run of deletions or of the missing symbol has started and not ended
   bool previous_is_start = false;  // ... with the record just before this one
   uint32_t run_list = 0;
   uint32_t run_first = 0;
   const auto endRun = [&](uint32_t past) {
      if (run_open) {
         append(row.lists[run_list], past - run_first == 1 ? std::to_string(run_first + 1) : std::to_string(run_first + 1) + "-" + std::to_string(past));
         row.cells[run_list] += past - run_first;
         run_open = false;
      }
   };
   uint32_t next_position = 0;  // what a record's position is at least
   for (const uint32_t* word = begin; word != end; ++word) {
      const uint32_t position = *word >> 9u;
      const bool close = ((*word >> 8u) & 1u) != 0;
      const auto byte = static_cast<uint8_t>(*word & 0xFFu);
      if (position < next_position || position >= positions) {
         return "a record whose position " + std::to_string(position) + " is not above the one before it or not inside the sequence";
      }
      next_position = position + 1;
      if (close) {
         if (!previous_is_start || byte != 0) {
            return "a close at position " + std::to_string(position) + " that does not follow a run start";
         }
         endRun(position);
         previous_is_start = false;
         continue;
      }
      if (!SymbolType::charToSymbol(static_cast<char>(byte)).has_value()) {
         return "a record at position " + std::to_string(position) + " whose byte " + std::to_string(byte) + " is no symbol of the alphabet";
      }
      const CellClass cell_class = classOfCell<SymbolType>(byte, reference[position]);
      if (cell_class == CellClass::SAME) {
         return "a record at position " + std::to_string(position) + " that holds the reference's symbol";
      }
      const uint32_t list = cell_class == CellClass::SUBSTITUTION ? 0u : cell_class == CellClass::DELETION ? 1u : cell_class == CellClass::MISSING ? 2u : 3u;
      const bool is_start = list == 1u || list == 2u;
      if (is_start && run_open && run_list == list) {
         return "a run start at position " + std::to_string(position) + " inside a run of its own kind";
      }
      endRun(position);
      previous_is_start = is_start;
      if (is_start) {
         run_open = true;
         run_list = list;
         run_first = position;
      } else {
         append(row.lists[list], std::string(1, reference[position]) + std::to_string(position + 1) + std::string(1, static_cast<char>(byte)));
         ++row.cells[list];
      }
   }
   endRun(positions);
   return "";
}

}  // namespace

template <typename SymbolType>
void MutationsPerSequence<SymbolType>::validateOrderByFields(const Database& database) const {
   checkOrderByFields({database.database_config.primary_key, "substitutionCount", "deletedPositions", "missingPositions", "ambiguousPositions"});
}

template <typename SymbolType>
QueryResult MutationsPerSequence<SymbolType>::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = actionName();
   const auto [name, store] = sequenceStoreOf<SymbolType>(database, sequence_name, "Database does not contain a sequence with name: ");
   const size_t total_count = selectedCount(database, bitmap_filter);
   CHECK_SILO_QUERY(total_count <= SEQUENCE_LIMIT, action_name + " action currently limited to " + std::to_string(SEQUENCE_LIMIT) + " sequences")
   requireUnsharded(database, action_name);
   std::string reference;  // as characters, what the device compares with and what the host re-checks against
   for (const auto symbol : store.reference_sequence) {
      reference += SymbolType::symbolToChar(symbol);
   }
   CHECK_SILO_QUERY(
      reference.size() <= SILO_GPU_MAX_DIFFERENCE_POSITIONS && total_count * reference.size() < (uint64_t{1} << 32u),
      action_name + " action: the sequence '" + name + "' has more than " + std::to_string(SILO_GPU_MAX_DIFFERENCE_POSITIONS) +
         " positions, or the selected sequences hold 2^32 characters or more"
   )
   const auto n = static_cast<uint32_t>(total_count);
   const auto positions = static_cast<uint32_t>(reference.size());
   constexpr size_t STATS = SILO_GPU_DIFFERENCE_STATS;
   const size_t head_words = n + 1u + n * STATS;  // the offsets, then the stats: fetched together

   std::vector<JsonValue> keys;          // of sequence 0 .. n - 1: partition order, then ascending row id
   std::vector<uint32_t> heads(head_words, 0u);  // (no selection or a sequence without positions: nothing launched, no word, no cell)
   std::vector<uint32_t> records;
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read and write it
      const bool launches = n != 0 && positions != 0;
      DevicePool& pool = database.partitions.front().pool;
      DeviceBuffer device_chars, device_reference, device_heads, device_scratch;
      DeviceBuffer device_records[2];  // of the first call and, where its capacity was too low, of the second
      SelectedSequences selection;     // (the row ids of every partition with selected rows, from its pool)
      launchAndWait([&] {
         if (launches) {
            device_chars = pool.acquire(static_cast<size_t>(n) * positions);
            device_reference = pool.acquire(positions);
            device_heads = pool.acquire(head_words * sizeof(uint32_t));
            device_scratch = pool.acquire(std::max<size_t>(sizeof(uint32_t), SILO_GPU_DIFFERENCES_SCRATCH_BYTES(n, positions)));
            checkGpu(silo_gpu_memcpy_h2d(device_reference.get(), reference.data(), positions, queryStream()), "silo_gpu_memcpy_h2d");
         }
         // reconstructSequence for a partition's rows at once, into their slice of the one buffer
         const SelectedSequences::Step gather = [&](const DatabasePartition& partition, const uint32_t* device_rows, uint32_t n_rows, size_t first_sequence) {
            checkGpu(
               silo_gpu_reconstruct_sequences(
                  partition.store, partition.template getSequenceStores<SymbolType>().at(name).seqstore_id, device_rows, n_rows,
                  device_chars.template as<char>() + first_sequence * positions, queryStream()
               ),
               "silo_gpu_reconstruct_sequences"
            );
         };
         selection.gather(database, bitmap_filter, n, action_name, false, launches ? gather : SelectedSequences::Step{});
         if (!launches) {
            return;
         }
         // rows of all partitions at once: one list, one pair of fetches
         uint32_t capacity = FIRST_WORDS_PER_ROW * n;
         for (size_t call = 0; call < 2; ++call) {
            DeviceBuffer& device_list = device_records[call];
            device_list = pool.acquire(static_cast<size_t>(capacity) * sizeof(uint32_t));
            checkGpu(
               silo_gpu_sequence_differences(
                  SymbolType::ABI_ALPHABET, device_chars.template as<char>(), n, positions, device_reference.template as<char>(), capacity,
                  device_heads.template as<uint32_t>(), device_heads.template as<uint32_t>() + n + 1u, device_list.template as<uint32_t>(),
                  device_scratch.get(), queryStream()
               ),
               "silo_gpu_sequence_differences"
            );
            const HostFetch head_fetch(device_heads.get(), head_words * sizeof(uint32_t), queryStream());
            const auto* host_heads = static_cast<const uint32_t*>(head_fetch.wait());
            const uint32_t total = host_heads[n];
            if (total > capacity) {
               if (call == 1) {  // the characters have not changed: the second total is the first
                  throw std::runtime_error(action_name + ": the device counted " + std::to_string(total) + " words where it had counted " + std::to_string(capacity));
               }
               capacity = total;  // exactly as many: the count is deterministic
               continue;
            }
            if (call == 1 && total != capacity) {
               throw std::runtime_error(action_name + ": the device counted " + std::to_string(total) + " words where it had counted " + std::to_string(capacity));
            }
            heads.assign(host_heads, host_heads + head_words);
            if (total != 0) {
               const HostFetch list_fetch(device_list.get(), static_cast<size_t>(total) * sizeof(uint32_t), queryStream());
               const auto* host_list = static_cast<const uint32_t*>(list_fetch.wait());
               records.assign(host_list, host_list + total);
            }
            break;
         }
      });
      keys = std::move(selection.keys);
   }
   Trace::mark("differences_on_host");

   // what came off the device is checked before it becomes rows: the offsets monotone and ending with the list, every row's words
   // sound (readRowDifferences), the cells they stand for equal to the row's four counts
   const auto broken = [&](const std::string& what) { return std::runtime_error(action_name + ": the device delivered " + what); };
   const uint32_t* offsets = heads.data();
   const uint32_t* stats = heads.data() + n + 1u;
   if (offsets[0] != 0 || offsets[n] != records.size()) {
      throw broken("offsets that do not span the list");
   }
   for (uint32_t r = 0; r < n; ++r) {
      if (offsets[r] > offsets[r + 1u]) {
         throw broken("offsets that decrease");
      }
   }
   static const char* const LIST_FIELDS[STATS] = {"substitutions", "deletions", "missing", "ambiguous"};
   static const char* const COUNT_FIELDS[STATS] = {"substitutionCount", "deletedPositions", "missingPositions", "ambiguousPositions"};
   const std::string& primary_key_column = database.database_config.primary_key;
   QueryResult results;
   results.query_result.reserve(n);
   for (uint32_t r = 0; r < n; ++r) {
      RowDifferences row;
      const std::string complaint = readRowDifferences<SymbolType>(records.data() + offsets[r], records.data() + offsets[r + 1u], reference, row);
      if (!complaint.empty()) {
         throw broken("for sequence " + std::to_string(r) + " " + complaint);
      }
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace(primary_key_column, std::move(keys[r]));
      entry.fields.emplace("sequenceName", name);
      for (size_t k = 0; k < STATS; ++k) {
         if (row.cells[k] != stats[r * STATS + k]) {
            throw broken(
               "for sequence " + std::to_string(r) + " records of " + std::to_string(row.cells[k]) + " cells in " + LIST_FIELDS[k] + " and a count of " +
               std::to_string(stats[r * STATS + k])
            );
         }
         entry.fields.emplace(LIST_FIELDS[k], std::move(row.lists[k]));
         entry.fields.emplace(COUNT_FIELDS[k], static_cast<int32_t>(row.cells[k]));
      }
   }
   return results;
}

template class MutationsPerSequence<Nucleotide>;
template class MutationsPerSequence<AminoAcid>;

template <typename SymbolType>
std::unique_ptr<Action> parseMutationsPerSequence(const json::Value& json) {
   const std::string action_name = MutationsPerSequence<SymbolType>::actionName();
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", action_name);
   CHECK_SILO_QUERY(
      (std::is_same_v<SymbolType, Nucleotide>) || sequence_name.has_value(), action_name + " action must contain the field sequenceName of type string (a gene)"
   )
   return std::make_unique<MutationsPerSequence<SymbolType>>(std::move(sequence_name));
}

template std::unique_ptr<Action> parseMutationsPerSequence<Nucleotide>(const json::Value& json);
template std::unique_ptr<Action> parseMutationsPerSequence<AminoAcid>(const json::Value& json);

// ---- CellCountDistribution (no counterpart in the reference) -------------------------------------------------
// The histogram of the selected rows' cell counts — the sum of the listed kinds of the four counts of MutationsPerSequence, taken
// from every store's kept table (K22) — in bins of binWidth, the last of maxBins bins open: what a user reads a threshold for the
// filter expression CellCount from.
void CellCountDistribution::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"from", "count"});
}

QueryResult CellCountDistribution::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence counted =
      alignedSequence(database, sequence_name, "CellCountDistribution: the field sequenceName: Database does not contain a sequence with name: ");
   requireUnsharded(database, "CellCountDistribution");
   QueryResult results;
   const size_t total_count = selectedCount(database, bitmap_filter);
   if (total_count == 0) {
      return results;
   }
   std::vector<uint64_t> bins(max_bins, 0);
   if (counted.positions == 0) {  // no cell to count: every row has the value 0, and no store a table
      bins[0] = total_count;
   } else {
      // nothing in here returns to the pool before the stream has been waited for: the launches write it
      const size_t bins_bytes = static_cast<size_t>(max_bins) * sizeof(uint64_t);
      const DeviceBuffer device_bins = database.partitions.front().pool.acquire(bins_bytes);
      launchAndWait([&] {
         checkGpu(silo_gpu_memset_async(device_bins.get(), 0, bins_bytes, queryStream()), "silo_gpu_memset_async");
         for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
            const DatabasePartition& partition = database.partitions[partition_id];
            if (partition.sequence_count == 0 || bitmap_filter[partition_id].cardinality() == 0) {
               continue;
            }
            const uint32_t* table = nullptr;
            checkGpu(
               silo_gpu_store_row_cell_counts(partition.store, counted.seqstoreOf(partition), &table, queryStream()), "silo_gpu_store_row_cell_counts"
            );
            checkGpu(
               silo_gpu_cell_count_histogram(
                  table, partition.rowWords(), partition.sequence_count, bitmap_filter[partition_id].bitset(), kinds_mask, bin_width, max_bins,
                  device_bins.as<uint64_t>(), queryStream()
               ),
               "silo_gpu_cell_count_histogram"
            );
         }
         const HostFetch fetch(device_bins.get(), bins_bytes, queryStream());
         std::memcpy(bins.data(), fetch.wait(), bins_bytes);
      });
   }
   uint64_t counted_rows = 0;
   for (const uint64_t count : bins) {
      counted_rows += count;
   }
   if (counted_rows != total_count) {
      throw std::runtime_error(
         "CellCountDistribution: the bins hold " + std::to_string(counted_rows) + " rows where the filters select " + std::to_string(total_count)
      );
   }
   for (uint32_t bin = 0; bin < max_bins; ++bin) {
      if (bins[bin] == 0) {
         continue;
      }
      // (bin + 1) * binWidth <= maxBins * binWidth <= 2^31: checked where the action is parsed
      const uint64_t from = static_cast<uint64_t>(bin) * bin_width;
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("from", static_cast<int32_t>(from));
      if (bin + 1u == max_bins) {
         entry.fields.emplace("to", std::nullopt);
      } else {
         entry.fields.emplace("to", static_cast<int32_t>(from + bin_width - 1u));
      }
      entry.fields.emplace("count", static_cast<int32_t>(bins[bin]));
   }
   return results;
}

std::unique_ptr<Action> parseCellCountDistribution(const json::Value& json) {
   const std::string action_name = "CellCountDistribution";
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", action_name);
   CHECK_SILO_QUERY(json.contains("cells"), action_name + " action: the field cells is required")
   const uint32_t kinds_mask = filter_expressions::parseCellKinds(
      json["cells"], action_name + " action: the field cells must be one of \"substitutions\", \"deletions\", \"missing\", \"ambiguous\" or a non-empty list "
                                   "of them without repeats"
   );
   const uint32_t bin_width = integerField(json, "binWidth", action_name, false, 1, INT32_MAX, "an integer of at least 1").value_or(1);
   const std::string bins_form = "an integer from 1 to " + std::to_string(CellCountDistribution::BIN_LIMIT);
   const uint32_t max_bins =
      integerField(json, "maxBins", action_name, false, 1, CellCountDistribution::BIN_LIMIT, bins_form).value_or(CellCountDistribution::DEFAULT_BINS);
   CHECK_SILO_QUERY(
      static_cast<uint64_t>(bin_width) * max_bins <= (uint64_t{1} << 31),
      action_name + " action: the fields binWidth and maxBins: their product must not exceed 2147483648, so that every bin's bounds are 32-bit numbers"
   )
   return std::make_unique<CellCountDistribution>(std::move(sequence_name), kinds_mask, bin_width, max_bins);
}

// ---- CellCountByRegion (no counterpart in the reference) -----------------------------------------------------
// Per named region of positions, the number of selected rows whose count of cells of the listed kinds inside the region lies within
// the region's bounds (K23): the amplicon drop-out table of a selection in one request.  Regions may overlap and K23's first entry
// takes disjoint ranges, so the regions are coloured into chunks of disjoint ones; disjoint chunks walk disjoint positions, so
// chunking adds launches and not cell work.
void CellCountByRegion::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"region", "positionFrom", "positionTo", "count"});
}

std::vector<std::vector<uint32_t>> CellCountByRegion::colourRegions(const std::vector<std::pair<uint32_t, uint32_t>>& ranges, size_t max_regions) {
   std::vector<uint32_t> by_start(ranges.size());
   std::iota(by_start.begin(), by_start.end(), 0u);
   std::stable_sort(by_start.begin(), by_start.end(), [&](uint32_t a, uint32_t b) { return ranges[a].first < ranges[b].first; });
   // taken by ascending start, a region overlaps none of a chunk exactly if it begins at or behind the end of the chunk's last one
   std::vector<std::vector<uint32_t>> chunks;
   for (const uint32_t region : by_start) {
      auto chunk = std::find_if(chunks.begin(), chunks.end(), [&](const std::vector<uint32_t>& candidate) {
         return candidate.size() < max_regions && ranges[candidate.back()].second <= ranges[region].first;
      });
      if (chunk == chunks.end()) {
         chunk = chunks.emplace(chunks.end());
      }
      chunk->push_back(region);
   }
   return chunks;
}

QueryResult CellCountByRegion::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const std::string action_name = "CellCountByRegion";
   const AlignedSequence counted =
      alignedSequence(database, sequence_name, action_name + ": the field sequenceName: Database does not contain a sequence with name: ");
   requireUnsharded(database, action_name);
   for (const Region& region : regions) {
      CHECK_SILO_QUERY(
         region.end <= counted.positions, action_name + ": the region '" + region.name + "': positionTo " + std::to_string(region.end) +
                                             " is past the end of the sequence '" + counted.name + "' (" + std::to_string(counted.positions) + " positions)"
      )
   }
   const size_t total_count = selectedCount(database, bitmap_filter);
   std::vector<uint64_t> counts(regions.size(), 0);
   if (total_count != 0) {
      uint32_t largest_row_words = 1;
      for (const DatabasePartition& partition : database.partitions) {
         largest_row_words = std::max(largest_row_words, partition.rowWords());
      }
      const size_t column_bytes = static_cast<size_t>(largest_row_words) * 64u * sizeof(uint32_t);
      const size_t chunk_regions = std::clamp<size_t>(REGION_VALUE_BUDGET_BYTES / column_bytes, 1, REGION_LIMIT);
      std::vector<std::pair<uint32_t, uint32_t>> ranges;
      for (const Region& region : regions) {
         ranges.emplace_back(region.first, region.end);
      }
      const std::vector<std::vector<uint32_t>> chunks = colourRegions(ranges, chunk_regions);
      size_t largest_chunk = 1;
      for (const std::vector<uint32_t>& chunk : chunks) {
         largest_chunk = std::max(largest_chunk, chunk.size());
      }
      // one array of counts in the regions' chunk order, so that a chunk's counts are neighbours: chunk_slot[c] is its first
      std::vector<size_t> chunk_slot;
      size_t slots = 0;
      for (const std::vector<uint32_t>& chunk : chunks) {
         chunk_slot.push_back(slots);
         slots += chunk.size();
      }
      // nothing in here returns to the pool before the stream has been waited for: the launches write it
      DevicePool& pool = database.partitions.front().pool;
      const size_t counts_bytes = slots * sizeof(uint64_t);
      const DeviceBuffer device_counts = pool.acquire(counts_bytes);
      const DeviceBuffer device_columns = pool.acquire(largest_chunk * column_bytes);
      const DeviceBuffer device_scratch = pool.acquire(SILO_GPU_REGION_VALUE_SCRATCH_BYTES(counted.positions));
      std::vector<uint64_t> chunked_counts(slots, 0);
      launchAndWait([&] {
         checkGpu(silo_gpu_memset_async(device_counts.get(), 0, counts_bytes, queryStream()), "silo_gpu_memset_async");
         for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
            const DatabasePartition& partition = database.partitions[partition_id];
            if (partition.sequence_count == 0 || bitmap_filter[partition_id].cardinality() == 0) {
               continue;
            }
            const uint64_t* filter = bitmap_filter[partition_id].isFull() ? nullptr : bitmap_filter[partition_id].bitset();
            for (size_t c = 0; c < chunks.size(); ++c) {
               std::vector<uint32_t> chunk_ranges;
               std::vector<uint32_t> chunk_bounds;
               for (const uint32_t region : chunks[c]) {
                  chunk_ranges.insert(chunk_ranges.end(), {regions[region].first, regions[region].end});
                  chunk_bounds.insert(chunk_bounds.end(), {regions[region].at_least, regions[region].at_most});
               }
               const auto n_columns = static_cast<uint32_t>(chunks[c].size());
               checkGpu(
                  silo_gpu_region_cell_values(
                     partition.store, counted.seqstoreOf(partition), chunk_ranges.data(), n_columns, kinds_mask, device_columns.as<uint32_t>(),
                     device_scratch.get(), queryStream()
                  ),
                  "silo_gpu_region_cell_values"
               );
               checkGpu(
                  silo_gpu_count_values(
                     device_columns.as<uint32_t>(), n_columns, partition.rowWords(), partition.sequence_count, filter, chunk_bounds.data(),
                     device_counts.as<uint64_t>() + chunk_slot[c], queryStream()
                  ),
                  "silo_gpu_count_values"
               );
            }
         }
         const HostFetch fetch(device_counts.get(), counts_bytes, queryStream());
         std::memcpy(chunked_counts.data(), fetch.wait(), counts_bytes);
      });
      for (size_t c = 0; c < chunks.size(); ++c) {
         for (size_t k = 0; k < chunks[c].size(); ++k) {
            counts[chunks[c][k]] = chunked_counts[chunk_slot[c] + k];
         }
      }
   }
   QueryResult results;
   for (size_t g = 0; g < regions.size(); ++g) {
      if (counts[g] > total_count) {
         throw std::runtime_error(
            action_name + ": the region '" + regions[g].name + "' counts " + std::to_string(counts[g]) + " rows where the filters select " +
            std::to_string(total_count)
         );
      }
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("region", regions[g].name);
      entry.fields.emplace("positionFrom", static_cast<int32_t>(regions[g].first + 1u));
      entry.fields.emplace("positionTo", static_cast<int32_t>(regions[g].end));
      entry.fields.emplace("count", static_cast<int32_t>(counts[g]));
      entry.fields.emplace("total", static_cast<int32_t>(total_count));
   }
   return results;
}

std::unique_ptr<Action> parseCellCountByRegion(const json::Value& json) {
   const std::string action_name = "CellCountByRegion";
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", action_name);
   CHECK_SILO_QUERY(json.contains("cells"), action_name + " action: the field cells is required")
   const uint32_t kinds_mask = filter_expressions::parseCellKinds(
      json["cells"], action_name + " action: the field cells must be one of \"substitutions\", \"deletions\", \"missing\", \"ambiguous\" or a non-empty list "
                                   "of them without repeats"
   );
   const std::string bound_form = "an integer from 0 to 4294967295";
   const std::string position_form = "an integer from 1 to 2147483647";
   const std::optional<uint32_t> at_least = integerField(json, "atLeast", action_name, false, 0, UINT32_MAX, bound_form);
   const std::optional<uint32_t> at_most = integerField(json, "atMost", action_name, false, 0, UINT32_MAX, bound_form);
   const std::string regions_form =
      action_name + " action: the field regions must be an array of 1 to " + std::to_string(CellCountByRegion::REGION_LIMIT) + " objects";
   CHECK_SILO_QUERY(json.contains("regions"), action_name + " action: the field regions is required")
   CHECK_SILO_QUERY(json["regions"].is_array(), regions_form)
   std::vector<CellCountByRegion::Region> regions;
   for (const json::Value& item : json["regions"].items()) {
      CHECK_SILO_QUERY(item.is_object() && regions.size() < CellCountByRegion::REGION_LIMIT, regions_form)
      CHECK_SILO_QUERY(
         item.contains("name") && item["name"].is_string(), action_name + " action: every region must have the field name of type string"
      )
      const std::string& name = item["name"].as_string();
      const std::string region_name = action_name + " action: the region '" + name + "'";
      CHECK_SILO_QUERY(
         std::none_of(regions.begin(), regions.end(), [&](const CellCountByRegion::Region& other) { return other.name == name; }),
         region_name + " is listed more than once: the names of the regions must be distinct"
      )
      // (integerField words its complaints as "<name> action: the field ...": the region's name stands where the action's would)
      const std::string region_fields = action_name + " action: the region '" + name + "':";
      const auto field = [&](std::string_view key, bool required, int64_t minimum, int64_t maximum, const std::string& form) {
         if (!item.contains(key)) {
            CHECK_SILO_QUERY(!required, region_fields + " the field " + std::string(key) + " is required")
            return std::optional<uint32_t>();
         }
         const json::Value& value = item[key];
         CHECK_SILO_QUERY(
            value.is_number_unsigned() && value.as_int64() >= minimum && value.as_int64() <= maximum,
            region_fields + " the field " + std::string(key) + (required ? " must be " : ", if present, must be ") + form
         )
         return std::optional<uint32_t>(value.as_uint32());
      };
      const uint32_t position_from = field("positionFrom", true, 1, INT32_MAX, position_form).value();
      const uint32_t position_to = field("positionTo", true, 1, INT32_MAX, position_form).value();
      CHECK_SILO_QUERY(position_from <= position_to, region_fields + " the field positionFrom may not be greater than positionTo")
      const std::optional<uint32_t> own_at_least = field("atLeast", false, 0, UINT32_MAX, bound_form);
      const std::optional<uint32_t> own_at_most = field("atMost", false, 0, UINT32_MAX, bound_form);
      // a region's own bounds replace the action's: both of them, so that a region's bounds are read in one place
      const bool own = own_at_least.has_value() || own_at_most.has_value();
      CHECK_SILO_QUERY(
         own || at_least.has_value() || at_most.has_value(),
         region_name + " has no bound: at least one of the fields atLeast and atMost is required, in the region or in the action"
      )
      regions.push_back(
         {name, position_from - 1u, position_to, (own ? own_at_least : at_least).value_or(0), (own ? own_at_most : at_most).value_or(UINT32_MAX)}
      );
   }
   CHECK_SILO_QUERY(!regions.empty(), regions_form)
   return std::make_unique<CellCountByRegion>(std::move(sequence_name), kinds_mask, std::move(regions));
}

}  // namespace silo::query_engine::actions
