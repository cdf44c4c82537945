// record_dump -- what the argument stage of the record entries (csrc/mwrt_records.cpp, linked as is) answers, as JSON: one
// object {"status", "message", "record"} per request line on stdin, `record` being the cut record as hex.  Built and run by
// tests/record_kit.py under ASan + UBSan for the four tests/test_*record_checks.py; needs no GPU.  HEX is the caller's
// record: the bytes are copied to a heap block of exactly their length, so a read beyond what the caller owns is a
// sanitiser report.
//
//   cut RECORD HEX                                    RECORD: mwrt_oe_step, ... -- the cut alone (status -1: below the minimum)
//   oe_step | oe_lm_prepare | oe_lm_solve | oe_cost | oe_gain | oe_product | whiten | whiten_apply   NPROF NLEV M HEX
//   nform_prepare | nform_solve | nform_cost | nform_char | nform_gain | select                      NPROF NLEV M HEX
//   obs_apply NPROF NLEV HEX
//   basis_project BASIS_NBLK NPROF M HEX
//   basis_expand NPROF HEX
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
    auto as = [&](auto* r) { return reinterpret_cast<decltype(r)>(caller.data()); };
    const size_t nargs = w.size() - 2;
    mwrt_oe_step step; mwrt_oe_lm lm; mwrt_oe_char ch; mwrt_obs_apply ob; mwrt_basis_apply ba; mwrt_obs_whiten wh;
    mwrt_oe_nform nf; mwrt_oe_nform_char nc; mwrt_oe_select sel;
    if (cmd == "cut" && nargs == 1) {
      const Record* recs[] = {&OE_STEP, &OE_LM, &OE_CHAR, &OBS_APPLY, &BASIS_APPLY, &OBS_WHITEN, &OE_NFORM, &OE_NFORM_CHAR,
                              &OE_SELECT};
      const Record* rec = nullptr;
      for (const Record* r : recs) if (w[1] == r->name) rec = r;
      if (!rec) { std::fprintf(stderr, "record_dump: unknown record '%s'\n", w[1].c_str()); return 2; }
      std::vector<unsigned char> out(rec->size, 0xEE);
      const bool ok = cut(*rec, caller.data(), out.data());
      answer(Refusal{ok ? MWRT_OK : MWRT_ERR_INVALID_ARGUMENT, ""}, out.data(), out.size());
    } else if (cmd == "oe_step" && nargs == 3) {
      answer(oe_step_args(num(1), (int32_t)num(2), (int32_t)num(3), as(&step), &step), &step, sizeof step);
    } else if ((cmd == "oe_lm_prepare" || cmd == "oe_lm_solve" || cmd == "oe_cost") && nargs == 3) {
      const LmCall call = cmd == "oe_lm_prepare" ? LmCall::Prepare : cmd == "oe_lm_solve" ? LmCall::Solve : LmCall::Cost;
      answer(oe_lm_args(call, num(1), (int32_t)num(2), (int32_t)num(3), as(&lm), &lm), &lm, sizeof lm);
    } else if ((cmd == "oe_gain" || cmd == "oe_product") && nargs == 3) {
      const CharCall call = cmd == "oe_gain" ? CharCall::Gain : CharCall::Product;
      answer(oe_char_args(call, num(1), (int32_t)num(2), (int32_t)num(3), as(&ch), &ch), &ch, sizeof ch);
    } else if ((cmd == "whiten" || cmd == "whiten_apply") && nargs == 3) {
      const WhitenCall call = cmd == "whiten" ? WhitenCall::Whiten : WhitenCall::Apply;
      answer(whiten_args(call, num(1), (int32_t)num(2), (int32_t)num(3), as(&wh), &wh), &wh, sizeof wh);
    } else if ((cmd == "nform_prepare" || cmd == "nform_solve" || cmd == "nform_cost") && nargs == 3) {
      const NfCall call = cmd == "nform_prepare" ? NfCall::Prepare : cmd == "nform_solve" ? NfCall::Solve : NfCall::Cost;
      answer(oe_nform_args(call, num(1), (int32_t)num(2), (int32_t)num(3), as(&nf), &nf), &nf, sizeof nf);
    } else if ((cmd == "nform_char" || cmd == "nform_gain") && nargs == 3) {
      const NfCharCall call = cmd == "nform_char" ? NfCharCall::Char : NfCharCall::Gain;
      answer(oe_nform_char_args(call, num(1), (int32_t)num(2), (int32_t)num(3), as(&nc), &nc), &nc, sizeof nc);
    } else if (cmd == "select" && nargs == 3) {
      answer(oe_select_args(num(1), (int32_t)num(2), (int32_t)num(3), as(&sel), &sel), &sel, sizeof sel);
    } else if (cmd == "obs_apply" && nargs == 2) {
      answer(obs_apply_args(num(1), (int32_t)num(2), as(&ob), &ob), &ob, sizeof ob);
    } else if (cmd == "basis_project" && nargs == 3) {
      answer(basis_project_args((int32_t)num(1), num(2), (int32_t)num(3), as(&ba), &ba), &ba, sizeof ba);
    } else if (cmd == "basis_expand" && nargs == 1) {
      answer(basis_expand_args(num(1), as(&ba), &ba), &ba, sizeof ba);
    } else {
      std::fprintf(stderr, "record_dump: unknown request '%s'\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
