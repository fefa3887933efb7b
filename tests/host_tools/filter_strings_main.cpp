// filter_strings_main.cpp — built by tests/test_region_cell_count_parse.py: one request body per line of stdin goes through
// silo::query_engine::Query; per line it prints the filter expression's toString, or the text of the exception — the body of the
// 400 response.  Parsing and toString touch no device.
#include <exception>
#include <iostream>
#include <string>
#include "query_engine.h"
int main() {
   std::string line;
   const silo::Database database;
   while (std::getline(std::cin, line)) {
      try {
         const silo::query_engine::Query query(line);
         std::cout << query.filter->toString(database) << "\n";
      } catch (const std::exception& error) {
         std::cout << error.what() << "\n";
      }
   }
   return 0;
}
