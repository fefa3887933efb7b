// mutation_rows_json_main.cpp — a stand-alone program over the writer of a Mutations query's response text
// (lapis-silo_amd/host/mutation_rows_json.h).  The writer's bytes are compared with an oracle built the slow way: one json::Value
// object per row (count, mutation, proportion, sequenceName) and dump(), the rows ordered by a plain comparator over materialised
// field values.  Built with -fsanitize=address,undefined and run by tests/test_mutation_rows_json.py.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <optional>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "json.h"
#include "mutation_rows_json.h"

namespace text = silo::query_engine::actions::mutation_rows;
namespace json = silo::json;

namespace {

int failures = 0;
int comparisons = 0;

void expect(bool condition, const std::string& what) {
   if (!condition) {
      fprintf(stderr, "FAILED: %s\n", what.c_str());
      ++failures;
   }
}

struct Row {  // as the device delivers it: the position is the one in the query's table
   uint32_t position;
   uint32_t symbol_index;
   uint32_t count;
   uint32_t total;
};

struct Store {
   std::string name;
   uint32_t offset;
   std::string reference;  // one character per position
   std::string fragment;
};

Store makeStore(const std::string& name, uint32_t offset, uint32_t length, const std::string& alphabet, uint32_t seed) {
   Store store{name, offset, std::string(length, '?'), text::sequenceNameFragment(name)};
   std::mt19937 rng(seed);
   for (char& c : store.reference) {
      c = alphabet[rng() % alphabet.size()];
   }
   return store;
}

using Order = std::vector<std::pair<std::string, bool>>;  // field name, ascending

/// The response the slow way.  `request`: indexes into `stores`, in request order.
std::string oracle(
   const std::vector<Row>& rows, const std::vector<Store>& stores, const std::vector<size_t>& request, const std::string& symbol_chars,
   const Order& order_by, std::optional<uint32_t> limit, std::optional<uint32_t> offset
) {
   struct Fields {
      int32_t count;
      std::string mutation;
      double proportion;
      std::string sequence_name;
   };
   std::vector<Fields> listed;  // stores in request order, positions ascending, symbols in alphabet order
   for (const size_t s : request) {
      const Store& store = stores[s];
      std::vector<Row> mine;
      for (const Row& row : rows) {
         if (row.position >= store.offset && row.position - store.offset < store.reference.size()) {
            mine.push_back(row);
         }
      }
      std::stable_sort(mine.begin(), mine.end(), [](const Row& a, const Row& b) {
         return a.position != b.position ? a.position < b.position : a.symbol_index < b.symbol_index;
      });
      for (const Row& row : mine) {
         const uint32_t position = row.position - store.offset;
         listed.push_back(
            {static_cast<int32_t>(row.count), store.reference[position] + std::to_string(position + 1) + symbol_chars[row.symbol_index],
             static_cast<double>(row.count) / static_cast<double>(row.total), store.name}
         );
      }
   }
   // Action::applySort: an index array 0, 1, 2, ..., a partial sort where the window ends before the rows do
   std::vector<uint32_t> order(listed.size());
   for (size_t i = 0; i < order.size(); ++i) {
      order[i] = static_cast<uint32_t>(i);
   }
   const size_t n = listed.size();
   if (!order_by.empty() && offset.value_or(0) < n) {
      const auto before = [&](uint32_t left, uint32_t right) {
         const Fields& a = listed[left];
         const Fields& b = listed[right];
         for (const auto& [name, ascending] : order_by) {
            if (name == "mutation" && a.mutation != b.mutation) {
               return (a.mutation < b.mutation) == ascending;
            }
            if (name == "proportion" && a.proportion != b.proportion) {
               return (a.proportion < b.proportion) == ascending;
            }
            if (name == "count" && a.count != b.count) {
               return (a.count < b.count) == ascending;
            }
         }
         return false;
      };
      const size_t window_end = limit.has_value() ? std::min<size_t>(n, static_cast<size_t>(*limit) + offset.value_or(0)) : n;
      if (window_end < n) {
         std::partial_sort(order.begin(), order.begin() + static_cast<std::ptrdiff_t>(window_end), order.end(), before);
      } else {
         std::sort(order.begin(), order.end(), before);
      }
   }
   const size_t first = std::min<size_t>(offset.value_or(0), n);
   const size_t count = limit.has_value() ? std::min<size_t>(*limit, n - first) : n - first;
   std::string out = "{\"queryResult\":[";
   for (size_t k = 0; k < count; ++k) {
      const Fields& fields = listed[order[first + k]];
      json::Value entry = json::Value::object();
      entry.set("count", json::Value(fields.count));
      entry.set("mutation", json::Value(fields.mutation));
      entry.set("proportion", json::Value(fields.proportion));
      entry.set("sequenceName", json::Value(fields.sequence_name));
      out += (k == 0 ? "" : ",") + entry.dump();
   }
   return out + "]}";
}

std::string written(
   const std::vector<Row>& rows, const std::vector<Store>& stores, const std::vector<size_t>& request, const std::string& symbol_chars,
   const Order& order_by, std::optional<uint32_t> limit, std::optional<uint32_t> offset
) {
   std::vector<text::StoreText> texts;
   for (const size_t s : request) {
      texts.push_back({stores[s].offset, static_cast<uint32_t>(stores[s].reference.size()), stores[s].reference.data(), stores[s].fragment});
   }
   std::vector<text::OrderBy> keys;
   for (const auto& [name, ascending] : order_by) {
      keys.push_back({name == "mutation" ? text::OrderKey::MUTATION : (name == "proportion" ? text::OrderKey::PROPORTION : text::OrderKey::COUNT), ascending});
   }
   // (an exact-size heap copy: a read past the rows is an error under the address sanitizer)
   const std::vector<Row> exact(rows.begin(), rows.end());
   return text::mutationRowsJson(exact.data(), exact.size(), texts, symbol_chars, keys, limit, offset);
}

std::string compare(
   const std::string& what, const std::vector<Row>& rows, const std::vector<Store>& stores, const std::vector<size_t>& request,
   const std::string& symbol_chars, const Order& order_by = {}, std::optional<uint32_t> limit = std::nullopt,
   std::optional<uint32_t> offset = std::nullopt
) {
   const std::string want = oracle(rows, stores, request, symbol_chars, order_by, limit, offset);
   const std::string got = written(rows, stores, request, symbol_chars, order_by, limit, offset);
   ++comparisons;
   if (got != want) {
      size_t at = 0;
      while (at < got.size() && at < want.size() && got[at] == want[at]) {
         ++at;
      }
      expect(false, what + ": differs from byte " + std::to_string(at) + "\n  got  " + got.substr(at > 40 ? at - 40 : 0, 160) + "\n  want " + want.substr(at > 40 ? at - 40 : 0, 160));
   }
   return got;
}

bool contains(const std::string& text, const std::string& part) {
   return text.find(part) != std::string::npos;
}

const std::string NUC = "-ACGT";
const std::string AA = "-ACDEFGHIKLMNPQRSTVWY*";
const std::vector<Order> ORDERS = {
   {},
   {{"mutation", true}},
   {{"mutation", false}},
   {{"proportion", true}},
   {{"proportion", false}},
   {{"count", true}},
   {{"count", false}},
   {{"count", false}, {"mutation", true}},
   {{"proportion", true}, {"count", false}},
   {{"proportion", false}, {"mutation", false}},
   {{"count", true}, {"proportion", false}, {"mutation", true}},
};

/// Every ordering and every window of limit and offset inside, at and past the row count.
void allOrdersAndWindows(const std::string& what, const std::vector<Row>& rows, const std::vector<Store>& stores, const std::vector<size_t>& request, const std::string& symbol_chars) {
   const auto n = static_cast<uint32_t>(rows.size());
   const std::vector<std::pair<std::optional<uint32_t>, std::optional<uint32_t>>> windows = {
      {std::nullopt, std::nullopt}, {0u, std::nullopt},      {1u, std::nullopt},   {n / 2, std::nullopt}, {n, std::nullopt},
      {n + 5, std::nullopt},        {std::nullopt, 1u},      {std::nullopt, n / 2}, {std::nullopt, n},     {std::nullopt, n + 5},
      {3u, 2u},                     {n / 3, n / 2},          {n, n / 2},           {0u, 3u},              {2u, n > 0 ? n - 1 : 0},
      {2u, n},                      {7u, n + 1},
   };
   for (size_t o = 0; o < ORDERS.size(); ++o) {
      for (size_t w = 0; w < windows.size(); ++w) {
         compare(what + ", order " + std::to_string(o) + ", window " + std::to_string(w), rows, stores, request, symbol_chars, ORDERS[o], windows[w].first, windows[w].second);
      }
   }
}

/// Rows at random cells of the stores, no cell twice; counts and totals from a few values, so that every key has ties.
std::vector<Row> randomRows(const std::vector<Store>& stores, const std::vector<size_t>& with_rows, size_t per_store, uint32_t n_symbols, uint32_t seed) {
   std::mt19937 rng(seed);
   std::vector<Row> rows;
   for (const size_t s : with_rows) {
      std::vector<uint32_t> cells;
      const auto length = static_cast<uint32_t>(stores[s].reference.size());
      while (cells.size() < std::min<size_t>(per_store, static_cast<size_t>(length) * n_symbols / 2)) {
         const uint32_t cell = rng() % (length * n_symbols);
         if (std::find(cells.begin(), cells.end(), cell) == cells.end()) {
            cells.push_back(cell);
         }
      }
      for (const uint32_t cell : cells) {
         const uint32_t total = 4u << (rng() % 3);  // 4, 8, 16
         rows.push_back({stores[s].offset + cell / n_symbols, cell % n_symbols, 1 + static_cast<uint32_t>(rng() % total), total});
      }
   }
   std::shuffle(rows.begin(), rows.end(), rng);
   return rows;
}

void noRowAndOneRow() {
   const std::vector<Store> stores = {makeStore("main", 0, 100, "ACGT", 1)};
   expect(compare("no row", {}, stores, {0}, NUC) == "{\"queryResult\":[]}", "no row gives an empty list");
   allOrdersAndWindows("no row", {}, stores, {0}, NUC);
   const std::vector<Row> one = {{41, 4, 3, 12}};
   const std::string body = compare("one row", one, stores, {0}, NUC);
   const std::string name = std::string(1, stores[0].reference[41]) + "42T";
   expect(body == "{\"queryResult\":[{\"count\":3,\"mutation\":\"" + name + "\",\"proportion\":0.25,\"sequenceName\":\"main\"}]}", "one row, written out: " + body);
   allOrdersAndWindows("one row", one, stores, {0}, NUC);
   expect(compare("no store asked for", one, stores, {}, NUC) == "{\"queryResult\":[]}", "no store, no row");
}

void deliveryOrder() {
   const std::vector<Store> stores = {makeStore("main", 0, 3'000, "ACGT", 2)};
   std::vector<Row> rows = randomRows(stores, {0}, 412, 5, 3);
   const std::string shuffled = compare("shuffled", rows, stores, {0}, NUC);
   std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.position != b.position ? a.position < b.position : a.symbol_index < b.symbol_index; });
   const std::string ascending = compare("in order", rows, stores, {0}, NUC);
   std::reverse(rows.begin(), rows.end());
   const std::string reversed = compare("reversed", rows, stores, {0}, NUC);
   expect(shuffled == ascending && reversed == ascending, "the response does not depend on the order of delivery");
   allOrdersAndWindows("412 rows reversed", rows, stores, {0}, NUC);
}

void severalStores() {
   // two stores asked for against their offset order, one of them twice, and one without a row
   std::vector<Store> two = {makeStore("first", 0, 500, "ACGT", 4), makeStore("second", 500, 300, "ACGT", 5)};
   const std::vector<Row> rows = randomRows(two, {0, 1}, 60, 5, 6);
   const std::string body = compare("two stores, second first", rows, two, {1, 0}, NUC);
   expect(body.find("\"second\"") < body.find("\"first\""), "stores come in request order");
   allOrdersAndWindows("two stores", rows, two, {1, 0}, NUC);
   compare("a store asked for twice", rows, two, {1, 0, 1}, NUC);
   compare("only the second asked for", rows, two, {1}, NUC);
   allOrdersAndWindows("a store without a row", randomRows(two, {1}, 40, 5, 7), two, {0, 1}, NUC);
   // twelve genes, amino-acid symbols with the stop codon
   std::vector<Store> twelve;
   uint32_t offset = 0;
   for (uint32_t g = 0; g < 12; ++g) {
      twelve.push_back(makeStore("gene" + std::to_string(g), offset, 50 + 37 * g, AA.substr(1), 10 + g));
      offset += 50 + 37 * g;
   }
   const std::vector<size_t> request = {7, 0, 11, 3, 4, 1, 10, 2, 9, 5, 8, 6};
   std::vector<Row> aa_rows = randomRows(twelve, {0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11}, 30, 22, 8);  // (gene5 has no row)
   aa_rows.push_back({twelve[3].offset + 9, 21, 5, 8});
   const std::string aa_body = compare("twelve stores", aa_rows, twelve, request, AA);
   expect(contains(aa_body, std::string(1, twelve[3].reference[9]) + "10*\""), "a stop codon is written as *");
   expect(!contains(aa_body, "\"gene5\""), "a store without a row writes none");
   allOrdersAndWindows("twelve stores", aa_rows, twelve, request, AA);
}

void numbersAndNames() {
   std::vector<Store> stores = {makeStore("main", 0, 29'903, "ACGT", 9)};
   stores[0].reference[0] = 'A';
   stores[0].reference[8] = 'C';
   stores[0].reference[9] = 'G';
   stores[0].reference[29'902] = 'T';
   const std::vector<Row> rows = {
      {29'902, 0, 7, 7},                         // count == total
      {9, 1, 1, 4'000'000'000u},                 // an exponent
      {8, 4, 3'000'000'000u, 4'000'000'000u},    // a count past 2^31
      {0, 4, 1, 3},
      {0, 2, 2, 3},
      {15'000, 3, 123'456, 10'000'000},
   };
   const std::string body = compare("numbers", rows, stores, {0}, NUC);
   expect(contains(body, "{\"count\":7,\"mutation\":\"T29903-\",\"proportion\":1.0,"), "count == total prints 1.0: " + body);
   expect(contains(body, "{\"count\":1,\"mutation\":\"G10A\",\"proportion\":2.5e-10,"), "1 / 4e9 prints with an exponent: " + body);
   expect(contains(body, "{\"count\":-1294967296,\"mutation\":\"C9T\",\"proportion\":0.75,"), "a count past 2^31 prints negative: " + body);
   expect(contains(body, "\"mutation\":\"A1C\"") && contains(body, "\"mutation\":\"A1T\""), "position 1: " + body);
   expect(body.find("A1C") < body.find("A1T") && body.find("A1T") < body.find("C9T") && body.find("C9T") < body.find("G10A") && body.find("G10A") < body.find("T29903-"),
          "positions ascending, symbols in alphabet order");
   allOrdersAndWindows("numbers", rows, stores, {0}, NUC);  // (the negative count sorts as the int32 it is written as)
   // a name that needs escaping: quote, backslash, a control character, a UTF-8 letter
   const std::string name = "S\"pi\\ke\x01\tg\xc3\xa9n";
   const std::vector<Store> named = {makeStore(name, 0, 40, AA.substr(1), 21), makeStore("plain", 40, 40, AA.substr(1), 22)};
   const std::string named_body = compare("escaped name", randomRows(named, {0, 1}, 12, 22, 23), named, {1, 0}, AA);
   expect(contains(named_body, "\"sequenceName\":\"S\\\"pi\\\\ke\\u0001\\tg\xc3\xa9n\"}"), "the name is escaped as json.h escapes it: " + named_body);
}

void manyTies() {
   // 2 000 rows with counts 1..4 of 4: long runs of equal keys through std::sort's and std::partial_sort's unstable paths
   const std::vector<Store> stores = {makeStore("main", 0, 1'000, "ACGT", 30)};
   std::mt19937 rng(31);
   std::vector<Row> rows;
   for (uint32_t position = 0; position < 1'000; ++position) {
      for (uint32_t symbol = 0; symbol < 2; ++symbol) {
         rows.push_back({position, symbol * 3, 1 + static_cast<uint32_t>(rng() % 4), 4});
      }
   }
   std::shuffle(rows.begin(), rows.end(), rng);
   for (const Order& order : ORDERS) {
      compare("ties, whole", rows, stores, {0}, NUC, order);
      compare("ties, window", rows, stores, {0}, NUC, order, 100u, 50u);
      compare("ties, long window", rows, stores, {0}, NUC, order, 1'500u, 499u);
   }
}

}  // namespace

int main() {
   noRowAndOneRow();
   deliveryOrder();
   severalStores();
   numbersAndNames();
   manyTies();
   if (failures != 0) {
      fprintf(stderr, "%d check(s) failed\n", failures);
      return 1;
   }
   printf("mutation rows json ok: %d responses compared\n", comparisons);
   return 0;
}
