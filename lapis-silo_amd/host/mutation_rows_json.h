// mutation_rows_json.h — the response text of a Mutations query, written from the selected rows in one pass.
//
// A pure function of plain values: no device, no database.  It gives the bytes that one json::Value object per row
// (count, mutation, proportion, sequenceName), ordered by Action::applySort and cut by applyOffsetAndLimit, would dump —
// tests/host_tools/mutation_rows_json_main.cpp builds exactly that and compares.
//
// Order of the rows before any orderByFields: the stores in request order, positions ascending, symbols in
// VALID_MUTATION_SYMBOLS order (mutations.cpp:190-229, 259-268).  The device appends rows in no particular order, so they are
// put in order by sorting one packed 64-bit key per row, (position << 5 | symbol_index) << 32 | index; a row is never copied.
#pragma once

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "json.h"

namespace silo::query_engine::actions::mutation_rows {

/// What the writer needs of one requested sequence store.  All of it is fixed once the store exists.
struct StoreText {
   uint32_t position_offset = 0;    // of the store's first position in the query's count table
   uint32_t length = 0;             // positions of the store
   const char* reference = nullptr; // `length` characters: the reference symbol of every position
   std::string_view name_fragment;  // ,"sequenceName":"<escaped name>"}  (sequenceNameFragment)
};

/// The end of every row of a store: its name is escaped once, when the store is made, not once per row.
inline std::string sequenceNameFragment(const std::string& sequence_name) {
   std::string out = ",\"sequenceName\":";
   json::Value::appendString(out, sequence_name);
   out.push_back('}');
   return out;
}

enum class OrderKey : uint8_t { MUTATION, PROPORTION, COUNT };
struct OrderBy {
   OrderKey key;
   bool ascending;
};

constexpr uint32_t SYMBOL_BITS = 5;                     // symbol_index < 32 (22 amino-acid symbols at most)
constexpr uint32_t MAX_POSITIONS = 1u << (32 - SYMBOL_BITS);
constexpr size_t NAME_CAPACITY = 12;                    // reference character, at most 10 digits, symbol character
constexpr size_t ROW_TEXT_CAPACITY = 10 + 11 + 13 + NAME_CAPACITY + 15 + 26;  // without the store's fragment

/// "<reference character><1-based position><symbol character>" at `out`; returns its end.
inline char* writeMutationName(char* out, char from, uint32_t position_in_store, char to) {
   *out++ = from;
   out = std::to_chars(out, out + 10, position_in_store + 1).ptr;
   *out++ = to;
   return out;
}

/// json::Value::appendDouble into a flat buffer: shortest round-trip form, ".0" where the text would read as an integer.
inline char* writeDouble(char* out, double value) {
   if (!std::isfinite(value)) {
      std::memcpy(out, "null", 4);
      return out + 4;
   }
   char* const end = std::to_chars(out, out + 24, value).ptr;
   bool integral = true;
   for (const char* c = out; c != end; ++c) {
      integral = integral && *c != '.' && *c != 'e' && *c != 'E';
   }
   if (!integral) {
      return end;
   }
   end[0] = '.';
   end[1] = '0';
   return end + 2;
}

/// The response body {"queryResult":[...]} of `n_rows` selected rows.  Row: any struct with uint32 position (in the query's
/// table), symbol_index, count and total — silo_gpu_mutation_row as the device delivers it.  `stores`: the requested stores in
/// request order (one named twice is written twice); a row outside all of them is not written.  `symbol_chars`: the characters
/// of VALID_MUTATION_SYMBOLS.
template <typename Row>
std::string mutationRowsJson(
   const Row* rows, size_t n_rows, const std::vector<StoreText>& stores, std::string_view symbol_chars, const std::vector<OrderBy>& order_by,
   std::optional<uint32_t> limit, std::optional<uint32_t> offset
) {
   if (n_rows > UINT32_MAX) {
      throw std::length_error("mutationRowsJson: more rows than a 32-bit index holds");
   }
   std::vector<uint64_t> keys(n_rows);
   for (size_t i = 0; i < n_rows; ++i) {
      if (rows[i].position >= MAX_POSITIONS || rows[i].symbol_index >= symbol_chars.size()) {
         throw std::out_of_range("mutationRowsJson: a row's position or symbol is outside the table");
      }
      keys[i] = (static_cast<uint64_t>(rows[i].position << SYMBOL_BITS | rows[i].symbol_index) << 32) | i;
   }
   std::sort(keys.begin(), keys.end());
   // the rows in output order: store << 32 | index (in `keys` itself where one store is asked for, the common case)
   std::vector<uint64_t> listed;
   listed.reserve(stores.size() == 1 ? 0 : n_rows);
   size_t max_fragment = 0;
   for (size_t s = 0; s < stores.size(); ++s) {
      const StoreText& store = stores[s];
      max_fragment = std::max(max_fragment, store.name_fragment.size());
      const uint64_t begin_key = static_cast<uint64_t>(store.position_offset) << (32 + SYMBOL_BITS);
      const uint64_t end_key = (static_cast<uint64_t>(store.position_offset) + store.length) << (32 + SYMBOL_BITS);
      const auto begin = std::lower_bound(keys.begin(), keys.end(), begin_key);
      const auto end = std::lower_bound(begin, keys.end(), end_key);
      if (stores.size() == 1) {
         keys.erase(end, keys.end());
         keys.erase(keys.begin(), begin);
         for (uint64_t& key : keys) {
            key &= UINT32_MAX;
         }
         listed.swap(keys);
         break;
      }
      for (auto key = begin; key != end; ++key) {
         listed.push_back(static_cast<uint64_t>(s) << 32 | (*key & UINT32_MAX));
      }
   }
   const size_t n_listed = listed.size();
   const auto rowOf = [&](uint32_t at) -> const Row& { return rows[listed[at] & UINT32_MAX]; };
   const auto storeOf = [&](uint32_t at) -> const StoreText& { return stores[listed[at] >> 32]; };
   const auto nameAt = [&](char* out, uint32_t at) {
      const Row& row = rowOf(at);
      const StoreText& store = storeOf(at);
      const uint32_t position = row.position - store.position_offset;
      return writeMutationName(out, store.reference[position], position, symbol_chars[row.symbol_index]);
   };

   // orderByFields: the comparator, the index array (0, 1, 2, ... over the rows in output order) and the std:: algorithms of
   // Action::applySort over the same values — a name compares as a string, a count as int32, a proportion as a double — so
   // ties fall where they fall there.
   std::vector<uint32_t> order(n_listed);
   for (size_t at = 0; at < n_listed; ++at) {
      order[at] = static_cast<uint32_t>(at);
   }
   const size_t first = std::min<size_t>(offset.value_or(0), n_listed);
   const size_t count = limit.has_value() ? std::min<size_t>(*limit, n_listed - first) : n_listed - first;
   if (!order_by.empty() && offset.value_or(0) < n_listed) {
      std::vector<char> names;  // only where a row's name is needed before the rows are written: NAME_CAPACITY bytes a row
      std::vector<uint8_t> name_length;
      for (const OrderBy& field : order_by) {
         if (field.key == OrderKey::MUTATION && names.empty()) {
            names.resize(n_listed * NAME_CAPACITY);
            name_length.resize(n_listed);
            for (size_t at = 0; at < n_listed; ++at) {
               char* const name = names.data() + at * NAME_CAPACITY;
               name_length[at] = static_cast<uint8_t>(nameAt(name, static_cast<uint32_t>(at)) - name);
            }
         }
      }
      const auto name = [&](uint32_t at) { return std::string_view(names.data() + at * NAME_CAPACITY, name_length[at]); };
      const auto proportion = [&](uint32_t at) { return static_cast<double>(rowOf(at).count) / static_cast<double>(rowOf(at).total); };
      const auto before = [&](uint32_t left, uint32_t right) {
         for (const OrderBy& field : order_by) {
            if (field.key == OrderKey::MUTATION) {
               const std::string_view a = name(left), b = name(right);
               if (!(a == b)) {
                  return (a < b) == field.ascending;
               }
            } else if (field.key == OrderKey::PROPORTION) {
               const double a = proportion(left), b = proportion(right);
               if (!(a == b)) {
                  return (a < b) == field.ascending;
               }
            } else {
               const auto a = static_cast<int32_t>(rowOf(left).count), b = static_cast<int32_t>(rowOf(right).count);
               if (!(a == b)) {
                  return (a < b) == field.ascending;
               }
            }
         }
         return false;
      };
      const size_t window_end = limit.has_value() ? std::min<size_t>(n_listed, static_cast<size_t>(*limit) + offset.value_or(0)) : n_listed;
      if (window_end < n_listed) {
         std::partial_sort(order.begin(), order.begin() + static_cast<std::ptrdiff_t>(window_end), order.end(), before);
      } else {
         std::sort(order.begin(), order.end(), before);
      }
   }

   // one buffer, sized for the longest text a row can have; every fragment is copied with its known length
   static constexpr std::string_view HEAD = "{\"queryResult\":[", TAIL = "]}";
   static constexpr std::string_view COUNT = "{\"count\":", MUTATION = ",\"mutation\":\"", PROPORTION = "\",\"proportion\":";
   std::string out;
   out.resize(HEAD.size() + TAIL.size() + count * (ROW_TEXT_CAPACITY + max_fragment));
   char* at = out.data();
   const auto put = [&at](std::string_view text) {
      std::memcpy(at, text.data(), text.size());
      at += text.size();
   };
   put(HEAD);
   for (size_t k = 0; k < count; ++k) {
      const uint32_t index = order[first + k];
      const Row& row = rowOf(index);
      // keys in the order of the reference's std::map: count < mutation < proportion < sequenceName
      if (k != 0) {
         *at++ = ',';
      }
      put(COUNT);
      at = std::to_chars(at, at + 11, static_cast<int32_t>(row.count)).ptr;  // (a count >= 2^31 prints negative, as the int32 field does)
      put(MUTATION);
      at = nameAt(at, index);
      put(PROPORTION);
      at = writeDouble(at, static_cast<double>(row.count) / static_cast<double>(row.total));
      put(storeOf(index).name_fragment);
   }
   put(TAIL);
   out.resize(static_cast<size_t>(at - out.data()));
   return out;
}

}  // namespace silo::query_engine::actions::mutation_rows
