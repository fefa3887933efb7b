// distance_actions.cpp — the actions that compare aligned sequences with each other (none has a counterpart in the reference: its
// clients fetch FastaAligned and compare the strings themselves), with their parsers:
//   DistanceMatrix        the rows FastaAligned would return, compared pairwise on the device (K10)
//   Clusters              the same rows, linked where they are within a distance bound; the connected components of the links on
//                         the device (K12)
//   MinimumSpanningTree   the same rows again: the minimum spanning forest of their distances within a bound, the tree that answers
//                         Clusters at every bound at once, on the device (K13)
//   NearestAmong          two selections: per row of the one its nearest rows of the other (K14)
//   NearestNeighbours     the rows of the whole database closest to one query sequence (K11); resolveQuerySequence, which
//                         WithinDistance shares with it
//   DistinctSequenceCounts  the selection's classes of equal sequences — distance 0 with N and ambiguity codes as characters —
//                         with their sizes (K20's owner table, K21)
// The first four gather and pack the rows they compare in the same way: that is here once, as PackedSelection, over the walk that
// every action on the selected rows' sequences shares (SelectedSequences, sequence_actions.cpp).
#include <algorithm>
#include <cstring>
#include <tuple>

#include "query_engine.h"

namespace silo::query_engine::actions {

// ---- what DistanceMatrix, Clusters, MinimumSpanningTree, NearestAmong and NearestNeighbours share -----------------------
namespace {

using storage::column::MetadataColumnPartition;

const std::string NON_NEGATIVE_INTEGER = "a non-negative integer";  // how the parsers word what maxDistance and minComparedPositions must be

constexpr uint32_t PACK_BATCH_ROWS = SILO_GPU_MAX_DISTANCE_ROWS;  // what one silo_gpu_distance_pack takes

/// The character buffer that a PackedSelection of up to n rows gathers into (pool of the first partition).
DeviceBuffer gatherBuffer(const Database& database, const AlignedSequence& sequence, uint32_t n) {
   return database.partitions.front().pool.acquire(std::max<size_t>(1, static_cast<size_t>(std::min(n, PACK_BATCH_ROWS)) * sequence.positions));
}

/// A sequence by name, as the five actions take it: none is the default nucleotide sequence.
AlignedSequence comparedSequence(const Database& database, const std::optional<std::string>& sequence_name) {
   return alignedSequence(database, sequence_name, "Database does not contain a sequence with name: ");
}

/// The n rows the filters select, numbered as SelectedSequences numbers them, as bit planes over positions on the device.  The
/// constructor reconstructs them in batches of PACK_BATCH_ROWS into device_chars (gatherBuffer) and packs every batch into its rows
/// of the ONE plane buffer (n * row_plane_words words, pool of the first partition), all enqueued on queryStream().  Every batch —
/// and every selection that is given the same device_chars — gathers into the SAME characters: they are in order on the stream, so
/// a gather starts after the pack before it has read them.  The object owns what those launches read and write (the planes; per
/// partition its row ids, from that partition's pool): like device_chars it must outlive the wait for the stream, so it is declared
/// before the launchAndWait whose launches read planes().  A sequence without positions: only the keys are collected, nothing is
/// launched.  `what`: who asks, for the messages.
class PackedSelection : private SelectedSequences {
  public:
   using SelectedSequences::keys;
   using SelectedSequences::numbering;

   PackedSelection(
      const Database& database, const std::vector<OperatorResult>& bitmap_filter, const AlignedSequence& sequence, uint32_t n, const DeviceBuffer& device_chars,
      const std::string& what, bool numbered = false
   ) {
      // of one row in the plane buffer of silo_gpu_distance_pack
      const size_t row_plane_words = static_cast<size_t>(SILO_GPU_DISTANCE_PLANES(sequence.alphabet)) * SILO_GPU_DISTANCE_WORDS(sequence.positions);
      const Step pack_batches = [&](const DatabasePartition& partition, const uint32_t* device_rows, uint32_t n_rows, size_t first_sequence) {
         for (uint32_t begin = 0; begin < n_rows; begin += PACK_BATCH_ROWS) {
            const uint32_t batch_rows = std::min(PACK_BATCH_ROWS, n_rows - begin);
            checkGpu(
               silo_gpu_reconstruct_sequences(
                  partition.store, sequence.seqstoreOf(partition), device_rows + begin, batch_rows, device_chars.as<char>(), queryStream()
               ),
               "silo_gpu_reconstruct_sequences"
            );
            checkGpu(
               silo_gpu_distance_pack(
                  sequence.alphabet, device_chars.as<char>(), batch_rows, sequence.positions,
                  device_planes.as<uint64_t>() + (first_sequence + begin) * row_plane_words, queryStream()
               ),
               "silo_gpu_distance_pack"
            );
         }
      };
      waitIfThrown([&] {  // (a constructor that throws destroys its members: not while a launch reads them)
         device_planes = database.partitions.front().pool.acquire(std::max<size_t>(8, n * row_plane_words * sizeof(uint64_t)));
         gather(database, bitmap_filter, n, what, numbered, sequence.positions == 0 ? Step{} : pack_batches);
      });
   }

   [[nodiscard]] const uint64_t* planes() const { return device_planes.as<uint64_t>(); }

  private:
   DeviceBuffer device_planes;
};

}  // namespace

// ---- DistanceMatrix --------------------------------------------------------------------------------------
// The pairwise distances of the selected sequences from the pair kernel (K10).
void DistanceMatrix::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"firstKey", "secondKey", "distance", "comparedPositions"});
}

QueryResult DistanceMatrix::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence sequence = comparedSequence(database, sequence_name);
   const size_t total_count = selectedCount(database, bitmap_filter);
   CHECK_SILO_QUERY(total_count <= SEQUENCE_LIMIT, "DistanceMatrix action currently limited to " + std::to_string(SEQUENCE_LIMIT) + " sequences")
   requireUnsharded(database, "DistanceMatrix");
   QueryResult results;
   if (total_count < 2) {
      return results;
   }
   const auto n = static_cast<uint32_t>(total_count);
   const uint32_t positions = sequence.positions;
   const size_t table_words = static_cast<size_t>(n) * n * 2u;

   std::vector<uint32_t> table(positions == 0 ? table_words : 0u, 0u);  // (a sequence without positions: nothing to compare, nothing launched)
   std::vector<JsonValue> keys;  // of sequence 0 .. n - 1: partition order, then ascending row id
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read it
      const DeviceBuffer device_chars = gatherBuffer(database, sequence, n);
      const DeviceBuffer device_table = database.partitions.front().pool.acquire(table_words * sizeof(uint32_t));
      PackedSelection selection(database, bitmap_filter, sequence, n, device_chars, "DistanceMatrix");
      launchAndWait([&] {
         if (positions != 0) {
            // rows of different partitions are compared with each other: one call over all of them, one table fetched
            checkGpu(
               silo_gpu_distance_pairs(sequence.alphabet, selection.planes(), n, positions, device_table.as<uint32_t>(), queryStream()),
               "silo_gpu_distance_pairs"
            );
            HostFetch fetch(device_table.get(), table_words * sizeof(uint32_t), queryStream());
            const auto* host = static_cast<const uint32_t*>(fetch.wait());
            table.assign(host, host + table_words);
         }
      });
      keys = std::move(selection.keys);
   }

   // maxDistance is applied here, before a row is built
   for (uint32_t i = 0; i < n; ++i) {
      for (uint32_t j = i + 1; j < n; ++j) {
         const size_t cell = (static_cast<size_t>(i) * n + j) * 2u;
         const uint32_t distance = table[cell];
         if (max_distance.has_value() && distance > *max_distance) {
            continue;
         }
         QueryResultEntry& entry = results.query_result.emplace_back();
         entry.fields.emplace("firstKey", keys[i]);
         entry.fields.emplace("secondKey", keys[j]);
         entry.fields.emplace("distance", static_cast<int32_t>(distance));
         entry.fields.emplace("comparedPositions", static_cast<int32_t>(table[cell + 1u]));
      }
   }
   return results;
}

std::unique_ptr<Action> parseDistanceMatrix(const json::Value& json) {
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", "DistanceMatrix");
   // (INT64_MIN: 2^63 and above, negative when read as int64, pass here and in NearestNeighbours; the other three parsers refuse them)
   const std::optional<uint32_t> max_distance = integerField(json, "maxDistance", "DistanceMatrix", false, INT64_MIN, INT32_MAX, NON_NEGATIVE_INTEGER);
   return std::make_unique<DistanceMatrix>(std::move(sequence_name), max_distance);
}

// ---- Clusters --------------------------------------------------------------------------------------------
// The single-linkage clusters of the selected sequences at a distance bound: the connected components of "distance <= maxDistance
// and comparedPositions >= minComparedPositions", from the bit-per-pair kernel and the components kernel (K12).
void Clusters::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"key", "cluster", "clusterSize"});
}

QueryResult Clusters::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence sequence = comparedSequence(database, sequence_name);
   const size_t total_count = selectedCount(database, bitmap_filter);
   CHECK_SILO_QUERY(total_count <= SEQUENCE_LIMIT, "Clusters action currently limited to " + std::to_string(SEQUENCE_LIMIT) + " sequences")
   requireUnsharded(database, "Clusters");
   QueryResult results;
   if (total_count == 0) {
      return results;
   }
   const auto n = static_cast<uint32_t>(total_count);
   const uint32_t positions = sequence.positions;

   // (a sequence without positions: nothing to compare, nothing launched — every pair has distance 0 and 0 positions compared)
   std::vector<uint32_t> labels(n, min_compared_positions == 0 ? 0u : UINT32_MAX);
   std::vector<JsonValue> keys;  // of sequence 0 .. n - 1, as DistanceMatrix numbers them
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read it
      DevicePool& pool = database.partitions.front().pool;
      const DeviceBuffer device_chars = gatherBuffer(database, sequence, n);
      const DeviceBuffer device_adjacency = pool.acquire(static_cast<size_t>(n) * SILO_GPU_ADJACENCY_WORDS(n) * sizeof(uint64_t));
      const DeviceBuffer device_labels = pool.acquire(n * sizeof(uint32_t));
      PackedSelection selection(database, bitmap_filter, sequence, n, device_chars, "Clusters");
      launchAndWait([&] {
         if (positions != 0) {
            // rows of different partitions are linked with each other: one bit matrix over all of them, one labelling, n labels fetched
            checkGpu(
               silo_gpu_distance_within(
                  sequence.alphabet, selection.planes(), n, positions, max_distance, min_compared_positions, device_adjacency.as<uint64_t>(), queryStream()
               ),
               "silo_gpu_distance_within"
            );
            checkGpu(
               silo_gpu_adjacency_components(device_adjacency.as<uint64_t>(), n, device_labels.as<uint32_t>(), nullptr, queryStream()),
               "silo_gpu_adjacency_components"
            );
            HostFetch fetch(device_labels.get(), n * sizeof(uint32_t), queryStream());
            const auto* host = static_cast<const uint32_t*>(fetch.wait());
            labels.assign(host, host + n);
         }
      });
      keys = std::move(selection.keys);
   }

   std::vector<uint32_t> sizes(n, 0);
   for (uint32_t i = 0; i < n; ++i) {
      if (labels[i] == UINT32_MAX) {  // (no positions and a bound on the compared positions: nothing is linked)
         labels[i] = i;
      }
      if (labels[i] >= n) {
         throw std::runtime_error("Clusters: a label names no selected sequence");
      }
      ++sizes[labels[i]];
   }
   // minClusterSize is applied here, before a row is built
   for (uint32_t i = 0; i < n; ++i) {
      const uint32_t size = sizes[labels[i]];
      if (size < min_cluster_size) {
         continue;
      }
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("key", keys[i]);
      entry.fields.emplace("cluster", keys[labels[i]]);
      entry.fields.emplace("clusterSize", static_cast<int32_t>(size));
   }
   return results;
}

std::unique_ptr<Action> parseClusters(const json::Value& json) {
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", "Clusters");
   const uint32_t max_distance = *integerField(json, "maxDistance", "Clusters", true, 0, INT32_MAX, NON_NEGATIVE_INTEGER);
   const uint32_t min_compared_positions = integerField(json, "minComparedPositions", "Clusters", false, 0, INT32_MAX, NON_NEGATIVE_INTEGER).value_or(0);
   const uint32_t min_cluster_size = integerField(json, "minClusterSize", "Clusters", false, 1, INT32_MAX, "an integer of at least 1").value_or(1);
   return std::make_unique<Clusters>(std::move(sequence_name), max_distance, min_compared_positions, min_cluster_size);
}

// ---- MinimumSpanningTree ---------------------------------------------------------------------------------
// The minimum spanning forest of the selected sequences under DistanceMatrix's distance — the single-linkage tree: cut at any d it
// leaves the clusters of Clusters at d — from the weights kernel, the one-block forest kernel and the listed-pairs kernel (K13).
void MinimumSpanningTree::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"firstKey", "secondKey", "distance", "comparedPositions"});
}

QueryResult MinimumSpanningTree::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence sequence = comparedSequence(database, sequence_name);
   const size_t total_count = selectedCount(database, bitmap_filter);
   CHECK_SILO_QUERY(
      total_count <= SEQUENCE_LIMIT, "MinimumSpanningTree action currently limited to " + std::to_string(SEQUENCE_LIMIT) + " sequences"
   )
   requireUnsharded(database, "MinimumSpanningTree");
   QueryResult results;
   if (total_count < 2) {
      return results;
   }
   const auto n = static_cast<uint32_t>(total_count);
   const uint32_t positions = sequence.positions;
   const size_t max_edges = n - 1u;

   struct Edge {
      uint32_t first;
      uint32_t second;
      uint32_t distance;
      uint32_t compared;
   };
   std::vector<Edge> edges;  // of the forest, by ascending key
   std::vector<JsonValue> keys;  // of sequence 0 .. n - 1, as DistanceMatrix numbers them
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read it
      DevicePool& pool = database.partitions.front().pool;
      const DeviceBuffer device_chars = gatherBuffer(database, sequence, n);
      // (a sequence without positions: nothing to compare, nothing launched, no matrix)
      const DeviceBuffer device_weights = pool.acquire(positions == 0 ? sizeof(uint32_t) : static_cast<size_t>(n) * n * sizeof(uint32_t));
      // what is fetched, in one piece: the keys of the edges, then the two counts of every edge, then the number of edges
      const size_t pairs_offset = max_edges * sizeof(uint64_t);
      const size_t count_offset = pairs_offset + max_edges * 2u * sizeof(uint32_t);
      const size_t result_bytes = count_offset + sizeof(uint64_t);
      const DeviceBuffer device_result = pool.acquire(result_bytes);
      auto* device_edges = device_result.as<uint64_t>();
      auto* device_pairs = reinterpret_cast<uint32_t*>(device_result.as<char>() + pairs_offset);
      auto* device_count = reinterpret_cast<uint32_t*>(device_result.as<char>() + count_offset);
      PackedSelection selection(database, bitmap_filter, sequence, n, device_chars, "MinimumSpanningTree");
      launchAndWait([&] {
         if (positions == 0) {
            // every pair has distance 0 and 0 positions compared: the star of sequence 0, or nothing at all
            for (uint32_t j = 1; min_compared_positions == 0 && j < n; ++j) {
               edges.push_back({0, j, 0, 0});
            }
            return;
         }
         // rows of different partitions are linked with each other: one matrix over all of them, one forest, its edges fetched
         checkGpu(
            silo_gpu_distance_weights(
               sequence.alphabet, selection.planes(), n, positions, max_distance.value_or(UINT32_MAX), min_compared_positions, device_weights.as<uint32_t>(),
               queryStream()
            ),
            "silo_gpu_distance_weights"
         );
         checkGpu(silo_gpu_spanning_forest(device_weights.as<uint32_t>(), n, device_edges, device_count, queryStream()), "silo_gpu_spanning_forest");
         checkGpu(
            silo_gpu_distance_listed_pairs(
               sequence.alphabet, selection.planes(), n, positions, device_edges, device_count, static_cast<uint32_t>(max_edges), device_pairs, queryStream()
            ),
            "silo_gpu_distance_listed_pairs"
         );
         HostFetch fetch(device_result.get(), result_bytes, queryStream());
         const auto* host = static_cast<const char*>(fetch.wait());
         uint32_t count = 0;
         std::memcpy(&count, host + count_offset, sizeof(count));
         if (count > max_edges) {
            throw std::runtime_error("MinimumSpanningTree: more edges than a forest has");
         }
         edges.reserve(count);
         for (uint32_t e = 0; e < count; ++e) {
            uint64_t key = 0;
            uint32_t counts[2];
            std::memcpy(&key, host + e * sizeof(uint64_t), sizeof(key));
            std::memcpy(counts, host + pairs_offset + e * sizeof(counts), sizeof(counts));
            const auto first = static_cast<uint32_t>(key >> SILO_GPU_SPANNING_KEY_ROW_BITS) & (SILO_GPU_MAX_SPANNING_ROWS - 1u);
            const auto second = static_cast<uint32_t>(key) & (SILO_GPU_MAX_SPANNING_ROWS - 1u);
            if (!(first < second && second < n)) {
               throw std::runtime_error("MinimumSpanningTree: an edge names no pair of selected sequences");
            }
            if (key >> SILO_GPU_SPANNING_KEY_WEIGHT_SHIFT != counts[0]) {
               throw std::runtime_error("MinimumSpanningTree: an edge's weight is not the distance of its pair");
            }
            edges.push_back({first, second, counts[0], counts[1]});
         }
      });
      keys = std::move(selection.keys);
   }

   for (const Edge& edge : edges) {
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("firstKey", keys[edge.first]);
      entry.fields.emplace("secondKey", keys[edge.second]);
      entry.fields.emplace("distance", static_cast<int32_t>(edge.distance));
      entry.fields.emplace("comparedPositions", static_cast<int32_t>(edge.compared));
   }
   return results;
}

std::unique_ptr<Action> parseMinimumSpanningTree(const json::Value& json) {
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", "MinimumSpanningTree");
   const std::optional<uint32_t> max_distance = integerField(json, "maxDistance", "MinimumSpanningTree", false, 0, INT32_MAX, NON_NEGATIVE_INTEGER);
   const uint32_t min_compared_positions =
      integerField(json, "minComparedPositions", "MinimumSpanningTree", false, 0, INT32_MAX, NON_NEGATIVE_INTEGER).value_or(0);
   return std::make_unique<MinimumSpanningTree>(std::move(sequence_name), max_distance, min_compared_positions);
}

// ---- NearestAmong ----------------------------------------------------------------------------------------
// For every selected sequence (a subject) its `neighbours` closest sequences among those a second filter selects (the candidates),
// under DistanceMatrix's distance, from the rectangle kernel and the per-row selection (K14).
void NearestAmong::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"key", "neighbourKey", "rank", "distance", "comparedPositions"});
}

QueryResult NearestAmong::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence sequence = comparedSequence(database, sequence_name);
   requireUnsharded(database, "NearestAmong");
   // the candidates: `among`, compiled and evaluated per partition as the top-level filter is; absent, the query's own filter
   std::vector<OperatorResult> among_filter;
   if (among != nullptr) {
      among_filter.reserve(database.partitions.size());
      for (const DatabasePartition& partition : database.partitions) {
         among_filter.push_back(operators::Operator::evaluate(among->compile(database, partition, filter_expressions::Expression::AmbiguityMode::NONE)));
      }
   }
   const std::vector<OperatorResult>& candidate_filter = among != nullptr ? among_filter : bitmap_filter;
   const size_t subject_count = selectedCount(database, bitmap_filter);
   const size_t candidate_count = selectedCount(database, candidate_filter);
   // both limits before anything is allocated
   CHECK_SILO_QUERY(subject_count <= SUBJECT_LIMIT, "NearestAmong action currently limited to " + std::to_string(SUBJECT_LIMIT) + " subjects")
   CHECK_SILO_QUERY(candidate_count <= CANDIDATE_LIMIT, "NearestAmong action currently limited to " + std::to_string(CANDIDATE_LIMIT) + " candidates")
   QueryResult results;
   if (subject_count == 0 || candidate_count == 0) {
      return results;
   }
   const auto m = static_cast<uint32_t>(subject_count);
   const auto n = static_cast<uint32_t>(candidate_count);
   const uint32_t k = neighbours;
   const uint32_t positions = sequence.positions;
   const size_t result_words = static_cast<size_t>(m) + static_cast<size_t>(m) * k * 3u;  // the counts, then the lists

   std::vector<uint32_t> self(m, UINT32_MAX);  // the candidate that is the same database row as subject s
   std::vector<uint32_t> result;               // a copy of what is fetched
   std::vector<JsonValue> subject_keys;    // of subject 0 .. m - 1, as DistanceMatrix numbers a selection
   std::vector<JsonValue> candidate_keys;  // of candidate 0 .. n - 1, numbered on its own in the same way
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read it
      DevicePool& pool = database.partitions.front().pool;
      const DeviceBuffer device_chars = gatherBuffer(database, sequence, std::max(m, n));
      // (a sequence without positions: nothing to compare, nothing launched, no cells)
      const DeviceBuffer device_cells = pool.acquire(positions == 0 ? sizeof(uint64_t) : static_cast<size_t>(m) * n * 2u * sizeof(uint32_t));
      const DeviceBuffer device_self = pool.acquire(m * sizeof(uint32_t));
      const DeviceBuffer device_result = pool.acquire(result_words * sizeof(uint32_t));
      // each side numbered on its own; both gather into the ONE character buffer: they are in order on the stream
      PackedSelection subjects(database, bitmap_filter, sequence, m, device_chars, "NearestAmong", true);
      PackedSelection candidates(database, candidate_filter, sequence, n, device_chars, "NearestAmong", true);
      launchAndWait([&] {
         // both numberings ascend by (partition, row id): one merge
         for (uint32_t s = 0, c = 0; s < m && c < n;) {
            if (subjects.numbering[s] == candidates.numbering[c]) {
               self[s++] = c++;
            } else if (subjects.numbering[s] < candidates.numbering[c]) {
               ++s;
            } else {
               ++c;
            }
         }
         if (positions != 0) {
            checkGpu(silo_gpu_memcpy_h2d(device_self.get(), self.data(), m * sizeof(uint32_t), queryStream()), "silo_gpu_memcpy_h2d");
            // rows of different partitions are compared with each other: one rectangle over both sides; it never leaves the device
            checkGpu(
               silo_gpu_distance_cross(
                  sequence.alphabet, subjects.planes(), m, candidates.planes(), n, positions, device_self.as<uint32_t>(), max_distance.value_or(UINT32_MAX),
                  min_compared_positions, device_cells.as<uint32_t>(), queryStream()
               ),
               "silo_gpu_distance_cross"
            );
            auto* device_counts = device_result.as<uint32_t>();
            checkGpu(
               silo_gpu_nearest_columns(device_cells.as<uint32_t>(), m, n, k, device_counts + m, device_counts, queryStream()), "silo_gpu_nearest_columns"
            );
            HostFetch fetch(device_result.get(), result_words * sizeof(uint32_t), queryStream());
            const auto* host = static_cast<const uint32_t*>(fetch.wait());
            result.assign(host, host + result_words);
         }
      });
      subject_keys = std::move(subjects.keys);
      candidate_keys = std::move(candidates.keys);
   }

   const auto addRow = [&](uint32_t subject, uint32_t rank, uint32_t candidate, uint32_t distance, uint32_t compared) {
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("key", subject_keys[subject]);
      entry.fields.emplace("neighbourKey", candidate_keys[candidate]);
      entry.fields.emplace("rank", static_cast<int32_t>(rank));
      entry.fields.emplace("distance", static_cast<int32_t>(distance));
      entry.fields.emplace("comparedPositions", static_cast<int32_t>(compared));
   };
   if (positions == 0) {
      // every pair has distance 0 and 0 positions compared: the first candidates by number other than the subject, or nothing at all
      for (uint32_t s = 0; min_compared_positions == 0 && s < m; ++s) {
         uint32_t rank = 0;
         for (uint32_t c = 0; c < n && rank < k; ++c) {
            if (c != self[s]) {
               addRow(s, ++rank, c, 0, 0);
            }
         }
      }
      return results;
   }
   for (uint32_t s = 0; s < m; ++s) {
      const uint32_t count = result[s];
      if (count > k) {
         throw std::runtime_error("NearestAmong: a subject lists more candidates than neighbours");
      }
      const uint32_t* list = result.data() + m + static_cast<size_t>(s) * k * 3u;
      for (uint32_t r = 0; r < count; ++r) {
         const uint32_t* entry = list + r * 3u;
         if (entry[0] >= n || entry[0] == self[s]) {
            throw std::runtime_error("NearestAmong: a listed candidate names no candidate, or the subject itself");
         }
         if (r != 0 && !(std::tie(entry[-2], entry[-3]) < std::tie(entry[1], entry[0]))) {
            throw std::runtime_error("NearestAmong: a subject's list does not ascend by (distance, candidate)");
         }
         addRow(s, r + 1u, entry[0], entry[1], entry[2]);
      }
   }
   return results;
}

std::unique_ptr<Action> parseNearestAmong(const json::Value& json) {
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", "NearestAmong");
   std::unique_ptr<filter_expressions::Expression> among;
   if (json.contains("among")) {
      CHECK_SILO_QUERY(json["among"].is_object(), "NearestAmong action: the field among, if present, must be a filter expression")
      try {
         among = filter_expressions::parseExpression(json["among"]);
      } catch (const QueryParseException& error) {
         throw QueryParseException(std::string("NearestAmong action: the field among is no filter expression: ") + error.what());
      }
   }
   const std::string neighbours_form = "an integer from 1 to " + std::to_string(NearestAmong::NEIGHBOUR_LIMIT);
   const uint32_t neighbours = integerField(json, "neighbours", "NearestAmong", false, 1, NearestAmong::NEIGHBOUR_LIMIT, neighbours_form)
                                  .value_or(NearestAmong::DEFAULT_NEIGHBOURS);
   const std::optional<uint32_t> max_distance = integerField(json, "maxDistance", "NearestAmong", false, 0, INT32_MAX, NON_NEGATIVE_INTEGER);
   const uint32_t min_compared_positions = integerField(json, "minComparedPositions", "NearestAmong", false, 0, INT32_MAX, NON_NEGATIVE_INTEGER).value_or(0);
   return std::make_unique<NearestAmong>(std::move(sequence_name), std::move(among), neighbours, max_distance, min_compared_positions);
}

// ---- NearestNeighbours -----------------------------------------------------------------------------------
// The rows of the whole database nearest to one query, from the per-row pass over the store's layout and the selection on the
// device (K11).
namespace {

/// The row of a partition whose primary key is `key`, read off the host copy of the column.  `what`: who asks, for the messages.
std::optional<uint32_t> rowOfKey(const MetadataColumnPartition& column, const json::Value& key, const std::string& what) {
   if (column.isStringLike()) {
      CHECK_SILO_QUERY(key.is_string(), what + ": the primary key column holds strings, primaryKey is " + key.dump())
      const std::optional<uint32_t> id = column.lookupId(key.as_string());
      if (!id.has_value()) {
         return std::nullopt;
      }
      const auto found = std::find(column.words.begin(), column.words.end(), *id);
      return found == column.words.end() ? std::nullopt : std::optional<uint32_t>(static_cast<uint32_t>(found - column.words.begin()));
   }
   CHECK_SILO_QUERY(column.type == config::ColumnType::INT, what + ": the primary key column is neither a string nor an int column")
   CHECK_SILO_QUERY(
      key.is_number_integer() && key.as_int64() > INT32_MIN && key.as_int64() <= INT32_MAX,
      what + ": the primary key column holds integers, primaryKey is " + key.dump()
   )
   const auto found = std::find(column.ints.begin(), column.ints.end(), static_cast<int32_t>(key.as_int64()));
   return found == column.ints.end() ? std::nullopt : std::optional<uint32_t>(static_cast<uint32_t>(found - column.ints.begin()));
}

}  // namespace

QuerySequence resolveQuerySequence(
   const Database& database, const AlignedSequence& compared, const std::optional<json::Value>& primary_key, const std::optional<std::string>& sequence,
   const std::string& what
) {
   const size_t positions = compared.positions;
   QuerySequence query;
   if (sequence.has_value()) {
      CHECK_SILO_QUERY(
         sequence->size() == positions, what + ": the field sequence has " + std::to_string(sequence->size()) + " characters, the sequence '" +
                                           compared.name + "' has " + std::to_string(positions)
      )
      query.characters = *sequence;
      return query;
   }
   const std::string& primary_key_column = database.database_config.primary_key;
   for (size_t partition_id = 0; partition_id < database.partitions.size() && query.own_partition == SIZE_MAX; ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      if (partition.sequence_count == 0) {
         continue;
      }
      if (const std::optional<uint32_t> row = rowOfKey(columnOf(partition, primary_key_column), *primary_key, what); row.has_value()) {
         query.own_partition = partition_id;
         query.own_row = *row;
      }
   }
   CHECK_SILO_QUERY(query.own_partition != SIZE_MAX, what + ": no sequence has the primary key " + primary_key->dump())
   query.characters.resize(positions);
   if (positions != 0) {
      const DatabasePartition& partition = database.partitions[query.own_partition];
      // the two buffers return to the pool when the gather has been waited for: the copy to the host is synchronous
      const DeviceBuffer device_row = partition.pool.acquire(sizeof(uint32_t));
      const DeviceBuffer device_chars = partition.pool.acquire(positions);
      waitIfThrown([&] {
         checkGpu(silo_gpu_memcpy_h2d(device_row.get(), &query.own_row, sizeof(uint32_t), queryStream()), "silo_gpu_memcpy_h2d");
         checkGpu(
            silo_gpu_reconstruct_sequences(partition.store, compared.seqstoreOf(partition), device_row.as<uint32_t>(), 1, device_chars.as<char>(), queryStream()),
            "silo_gpu_reconstruct_sequences"
         );
         checkGpu(silo_gpu_memcpy_d2h(query.characters.data(), device_chars.get(), positions, queryStream()), "silo_gpu_memcpy_d2h");
      });
   }
   return query;
}

void NearestNeighbours::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"primaryKey", "distance", "comparedPositions"});
}

QueryResult NearestNeighbours::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence compared = comparedSequence(database, sequence_name);
   requireUnsharded(database, "NearestNeighbours");
   const std::string& primary_key_column = database.database_config.primary_key;

   struct Hit {
      uint32_t distance;
      size_t partition;
      uint32_t row;
      uint32_t compared;
   };
   std::vector<Hit> hits;
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read it
      std::vector<DeviceBuffer> live;  // per partition: the table, two scratches, the list
      launchAndWait([&] {
         // the query's characters: the literal string, or the row of that key gathered from its partition (and left out there)
         const QuerySequence resolved = resolveQuerySequence(database, compared, primary_key, sequence, "NearestNeighbours action");
         const std::string& query = resolved.characters;
         const size_t own_partition = resolved.own_partition;
         const uint32_t own_row = resolved.own_row;

         const size_t list_words = static_cast<size_t>(neighbours) * 3u + 1u;  // the list, then its length
         for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
            const DatabasePartition& partition = database.partitions[partition_id];
            const OperatorResult& filter = bitmap_filter[partition_id];
            const uint32_t selected = partition.sequence_count == 0 ? 0 : filter.cardinality();
            if (selected == 0) {
               continue;
            }
            // a filter that selects every row is passed as NULL (no all-ones bitset is made for it)
            const uint64_t* filter_bits = selected == partition.sequence_count ? nullptr : filter.bitset();
            auto* table = live.emplace_back(partition.pool.acquire(static_cast<size_t>(partition.rowWords()) * 64u * 2u * sizeof(uint32_t))).as<uint32_t>();
            void* table_scratch = live.emplace_back(partition.pool.acquire(SILO_GPU_QUERY_DISTANCE_SCRATCH_BYTES(compared.positions))).get();
            void* select_scratch = live.emplace_back(partition.pool.acquire(SILO_GPU_NEAREST_ROWS_SCRATCH_BYTES)).get();
            auto* list = live.emplace_back(partition.pool.acquire(list_words * sizeof(uint32_t))).as<uint32_t>();
            checkGpu(
               silo_gpu_query_distances(partition.store, compared.seqstoreOf(partition), query.data(), table, table_scratch, queryStream()),
               "silo_gpu_query_distances"
            );
            checkGpu(
               silo_gpu_nearest_rows(
                  table, filter_bits, partition.sequence_count, partition_id == own_partition ? own_row : UINT32_MAX, max_distance.value_or(UINT32_MAX),
                  neighbours, list, list + list_words - 1u, select_scratch, queryStream()
               ),
               "silo_gpu_nearest_rows"
            );
            HostFetch fetch(list, list_words * sizeof(uint32_t), queryStream());
            const auto* host = static_cast<const uint32_t*>(fetch.wait());
            const uint32_t count = std::min(host[list_words - 1u], neighbours);
            for (uint32_t i = 0; i < count; ++i) {
               hits.push_back({host[3u * i + 1u], partition_id, host[3u * i], host[3u * i + 2u]});
            }
         }
      });
   }

   // every partition's list is ascending by (distance, row): the merge order is (distance, partition, row)
   std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) {
      return std::tie(a.distance, a.partition, a.row) < std::tie(b.distance, b.partition, b.row);
   });
   if (hits.size() > neighbours) {
      hits.resize(neighbours);
   }
   QueryResult results;
   results.query_result.reserve(hits.size());
   for (const Hit& hit : hits) {
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("primaryKey", columnOf(database.partitions[hit.partition], primary_key_column).jsonOfRow(hit.row));
      entry.fields.emplace("distance", static_cast<int32_t>(hit.distance));
      entry.fields.emplace("comparedPositions", static_cast<int32_t>(hit.compared));
   }
   return results;
}

std::unique_ptr<Action> parseNearestNeighbours(const json::Value& json) {
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", "NearestNeighbours");
   CHECK_SILO_QUERY(
      json.contains("primaryKey") != json.contains("sequence"), "NearestNeighbours action: exactly one of the fields primaryKey and sequence must be given"
   )
   std::optional<json::Value> primary_key;
   std::optional<std::string> sequence;
   if (json.contains("primaryKey")) {
      CHECK_SILO_QUERY(
         json["primaryKey"].is_string() || json["primaryKey"].is_number_integer(), "NearestNeighbours action: the field primaryKey must be a string or an integer"
      )
      primary_key = json["primaryKey"];
   } else {
      CHECK_SILO_QUERY(json["sequence"].is_string(), "NearestNeighbours action: the field sequence must be of type string")
      sequence = json["sequence"].as_string();
   }
   const std::string neighbours_form = "an integer from 1 to " + std::to_string(NearestNeighbours::NEIGHBOUR_LIMIT);
   const uint32_t neighbours = integerField(json, "neighbours", "NearestNeighbours", false, 1, NearestNeighbours::NEIGHBOUR_LIMIT, neighbours_form)
                                  .value_or(NearestNeighbours::DEFAULT_NEIGHBOURS);
   // (INT64_MIN: see parseDistanceMatrix)
   const std::optional<uint32_t> max_distance = integerField(json, "maxDistance", "NearestNeighbours", false, INT64_MIN, INT32_MAX, NON_NEGATIVE_INTEGER);
   return std::make_unique<NearestNeighbours>(std::move(sequence_name), std::move(primary_key), std::move(sequence), neighbours, max_distance);
}

// ---- DistinctSequenceCounts ------------------------------------------------------------------------------
// The largest classes of rows with equal aligned sequences among the selected rows, each with its size and its representative's
// primary key — the weights of the rows the filter expression DistinctSequences keeps — from K20's owner table, the two class-count
// passes and the selection of the smallest keys (K21).
void DistinctSequenceCounts::validateOrderByFields(const Database& /*database*/) const {
   checkOrderByFields({"primaryKey", "count"});
}

QueryResult DistinctSequenceCounts::execute(const Database& database, std::vector<OperatorResult> bitmap_filter) const {
   const AlignedSequence compared =
      alignedSequence(database, sequence_name, "DistinctSequenceCounts: the field sequenceName: Database does not contain a sequence with name: ");
   CHECK_SILO_QUERY(
      database.shard_world <= 1, "DistinctSequenceCounts is not supported on a sharded database yet: the rows of a selection on the other ranks take part in "
                                 "the choice, and a row's number in the database is not known to a rank"
   )
   // every partition that has rows, with the number of its first row in the database: the classes are those of all of them
   std::vector<operators::DistinctTable::Part> parts;
   std::vector<size_t> partition_of_part;
   std::vector<uint32_t> first_rows;
   uint64_t database_rows = 0;
   for (size_t partition_id = 0; partition_id < database.partitions.size(); ++partition_id) {
      const DatabasePartition& partition = database.partitions[partition_id];
      if (database_rows + partition.sequence_count >= (uint64_t{1} << 32) - 1) {
         throw QueryCompilationException(
            "DistinctSequenceCounts numbers the rows of the database with 32 bits: it needs a database of fewer than 2^32 - 1 rows"
         );
      }
      if (partition.sequence_count != 0) {
         parts.push_back({&partition, compared.seqstoreOf(partition), static_cast<uint32_t>(database_rows)});
         partition_of_part.push_back(partition_id);
         first_rows.push_back(static_cast<uint32_t>(database_rows));
      }
      database_rows += partition.sequence_count;
   }
   QueryResult results;
   if (selectedCount(database, bitmap_filter) == 0) {
      return results;
   }
   const auto capacity = static_cast<uint32_t>(database_rows);  // of the list of keys: no more classes than rows
   const uint32_t k = max_classes;
   // what is fetched, in one piece: the k smallest keys, then how many of them there are and how many classes were listed
   const size_t count_offset = static_cast<size_t>(k) * sizeof(uint64_t);
   const size_t result_bytes = count_offset + 2u * sizeof(uint32_t);

   std::vector<uint64_t> keys;  // ascending: by count descending, then by the representative's row in the database
   {
      // nothing in here returns to the pool before the stream has been waited for: the launches read and write it
      DevicePool& pool = database.partitions.front().pool;
      std::vector<DeviceBuffer> live;  // the uploaded parts and the owner table
      const DeviceBuffer device_keys = pool.acquire(static_cast<size_t>(capacity) * sizeof(uint64_t));
      const DeviceBuffer device_scratch = pool.acquire(SILO_GPU_SMALLEST_KEYS_SCRATCH_BYTES);
      const DeviceBuffer device_result = pool.acquire(result_bytes);
      DeviceBuffer device_counts;  // (sized with the table)
      auto* device_out = device_result.as<uint64_t>();
      auto* device_out_count = reinterpret_cast<uint32_t*>(device_result.as<char>() + count_offset);
      uint32_t* device_n_keys = device_out_count + 1;
      launchAndWait([&] {
         const operators::DistinctTable built = operators::buildDistinctTable(
            parts, database_rows, [&](size_t part) { return bitmap_filter[partition_of_part[part]].bitset(); },
            [&](size_t bytes) { return live.emplace_back(pool.acquire(std::max<size_t>(bytes, 1))).get(); }, "DistinctSequenceCounts"
         );
         device_counts = pool.acquire(SILO_GPU_DISTINCT_COUNTS_BYTES(built.slots));
         checkGpu(silo_gpu_memset_async(device_counts.get(), 0, SILO_GPU_DISTINCT_COUNTS_BYTES(built.slots), queryStream()), "silo_gpu_memset_async");
         checkGpu(silo_gpu_memset_async(device_n_keys, 0, sizeof(uint32_t), queryStream()), "silo_gpu_memset_async");
         for (uint32_t part = 0; part < built.n_parts; ++part) {
            checkGpu(
               silo_gpu_distinct_count(
                  built.table, built.slots, device_counts.as<uint32_t>(), built.device_parts, built.n_parts, part, built.filters[part], queryStream()
               ),
               "silo_gpu_distinct_count"
            );
         }
         for (uint32_t part = 0; part < built.n_parts; ++part) {
            checkGpu(
               silo_gpu_distinct_classes(
                  built.table, built.slots, device_counts.as<uint32_t>(), built.device_parts, built.n_parts, part, built.filters[part], min_count,
                  device_keys.as<uint64_t>(), capacity, device_n_keys, queryStream()
               ),
               "silo_gpu_distinct_classes"
            );
         }
         checkGpu(
            silo_gpu_smallest_keys(device_keys.as<uint64_t>(), device_n_keys, capacity, k, device_out, device_out_count, device_scratch.get(), queryStream()),
            "silo_gpu_smallest_keys"
         );
         HostFetch fetch(device_result.get(), result_bytes, queryStream());
         HostFetch overflow_fetch(static_cast<const uint32_t*>(built.table) + built.slots, sizeof(uint32_t), queryStream());
         const auto* host = static_cast<const char*>(fetch.wait());
         uint32_t counters[2];  // the keys selected, the classes listed
         std::memcpy(counters, host + count_offset, sizeof(counters));
         uint32_t overflow = 0;
         std::memcpy(&overflow, overflow_fetch.wait(), sizeof(overflow));
         if (overflow != 0) {
            throw std::runtime_error("DistinctSequenceCounts: a selected row was not found in the owner table");
         }
         if (counters[1] > capacity) {
            throw std::runtime_error("DistinctSequenceCounts: more classes than the database has rows");
         }
         if (counters[0] != std::min(counters[1], k)) {
            throw std::runtime_error("DistinctSequenceCounts: the selection of the largest classes lost or made up a class");
         }
         keys.resize(counters[0]);
         std::memcpy(keys.data(), host, keys.size() * sizeof(uint64_t));
      });
   }

   std::sort(keys.begin(), keys.end());
   const std::string& primary_key_column = database.database_config.primary_key;
   results.query_result.reserve(keys.size());
   for (const uint64_t key : keys) {
      const auto global_row = static_cast<uint32_t>(key);
      const uint32_t count = 0xFFFFFFFFu - static_cast<uint32_t>(key >> 32);
      // the part is the last one whose first row is <= the row
      const size_t part = static_cast<size_t>(std::upper_bound(first_rows.begin(), first_rows.end(), global_row) - first_rows.begin());
      if (part == 0 || global_row - first_rows[part - 1] >= parts[part - 1].partition->sequence_count || count == 0) {
         throw std::runtime_error("DistinctSequenceCounts: a key names no row of the database, or a class without rows");
      }
      const DatabasePartition& partition = *parts[part - 1].partition;
      QueryResultEntry& entry = results.query_result.emplace_back();
      entry.fields.emplace("count", static_cast<int32_t>(count));
      entry.fields.emplace("primaryKey", columnOf(partition, primary_key_column).jsonOfRow(global_row - first_rows[part - 1]));
   }
   return results;
}

std::unique_ptr<Action> parseDistinctSequenceCounts(const json::Value& json) {
   std::optional<std::string> sequence_name = optionalStringField(json, "sequenceName", "DistinctSequenceCounts");
   const uint32_t min_count = integerField(json, "minCount", "DistinctSequenceCounts", false, 1, INT32_MAX, "an integer of at least 1").value_or(1);
   const std::string classes_form = "an integer from 1 to " + std::to_string(DistinctSequenceCounts::CLASS_LIMIT);
   const uint32_t max_classes = integerField(json, "maxClasses", "DistinctSequenceCounts", false, 1, DistinctSequenceCounts::CLASS_LIMIT, classes_form)
                                   .value_or(DistinctSequenceCounts::DEFAULT_CLASSES);
   return std::make_unique<DistinctSequenceCounts>(std::move(sequence_name), min_count, max_classes);
}

}  // namespace silo::query_engine::actions
