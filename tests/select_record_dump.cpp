// select_record_dump -- what the argument stage of the observation selection (csrc/mwrt_records.cpp oe_select_args, linked
// as is) answers, as JSON: one object {"status", "message", "record"} per request line on stdin, `record` being the cut
// record as hex.  Built and run by tests/test_select_record_checks.py under ASan + UBSan; needs no GPU.  HEX is the caller's
// record: the bytes are copied to a heap block of exactly their length, so a read beyond what the caller owns is a
// sanitiser report.
//
//   cut HEX                      the cut alone (status -1: below the minimum)
//   select NPROF NLEV M HEX
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../mwr_fast_forward_operators_and_lbls_amd/csrc/mwrt_records.h"

using namespace mwrt::records;

static void answer(const Refusal& no, const void* rec, size_t size) {
  std::string msg;
  for (char ch : no.message) { if (ch == '"' || ch == '\\') msg += '\\'; msg += ch; }
  std::printf("{\"status\": %d, \"message\": \"%s\", \"record\": \"", no.status, msg.c_str());
  for (size_t i = 0; i < size; ++i) std::printf("%02x", static_cast<const unsigned char*>(rec)[i]);
  std::printf("\"}\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<std::string> w;
    for (std::string x; in >> x;) w.push_back(x);
    if (w.empty()) continue;
    const std::string cmd = w.front(), hex = w.back();
    std::vector<unsigned char> caller(hex.size() / 2);
    for (size_t i = 0; i < caller.size(); ++i) caller[i] = (unsigned char)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
    auto num = [&](size_t i) { return std::stoll(w.at(i)); };
    const size_t nargs = w.size() - 2;
    mwrt_oe_select rec;
    if (cmd == "cut" && nargs == 0) {
      std::vector<unsigned char> out(OE_SELECT.size, 0xEE);
      const bool ok = cut(OE_SELECT, caller.data(), out.data());
      answer(Refusal{ok ? MWRT_OK : MWRT_ERR_INVALID_ARGUMENT, ""}, out.data(), out.size());
    } else if (cmd == "select" && nargs == 3) {
      answer(oe_select_args(num(1), (int32_t)num(2), (int32_t)num(3), reinterpret_cast<const mwrt_oe_select*>(caller.data()), &rec),
             &rec, sizeof rec);
    } else {
      std::fprintf(stderr, "select_record_dump: unknown request '%s'\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
