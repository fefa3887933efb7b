// parse_messages_main.cpp — built with -fsanitize=address,undefined by tests/test_action_parse_messages.py: one request body per
// line of stdin goes through silo::query_engine::Query (the JSON parser, the Expression and the Action builders); per line it prints
// `ok`, or the text of the exception — the body of the 400 response.  Parsing touches no device.
#include <exception>
#include <iostream>
#include <string>
#include "query_engine.h"
int main() {
   std::string line;
   while (std::getline(std::cin, line)) {
      try {
         const silo::query_engine::Query query(line);
         std::cout << "ok\n";
      } catch (const std::exception& error) {
         std::cout << error.what() << "\n";
      }
   }
   return 0;
}
