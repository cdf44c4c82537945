// mwrt_records.h -- the argument stage of the entries that take a versioned record (a struct that starts with its own
// struct_size): everything they decide from their arguments alone.  Plain C++17 over include/mwrt.h, no HIP in it (the
// rule of mwrt_plan.h): tests/record_dump.cpp links mwrt_records.cpp as is under ASan + UBSan, without a GPU.
//
// The record convention, stated once: a field is read if and only if it lies wholly below min(struct_size, sizeof); every
// other field -- at or beyond the caller's struct_size, or one it ends inside -- is taken as NULL / 0.  A struct_size
// below the record's documented minimum is refused.
//
// A stage function takes the entry's scalar arguments, what it needs of its handle's dimensions and the caller's record
// (not null).  It writes the cut record to *r and returns an empty Refusal, or the status and the message of the first
// check that fails, in the order the entry documents: struct_size, signs and ranges, nblk, reserved fields, modes,
// pointers (required, paired, aliased, "nothing to do"), the row window, the limits of mwrt.h.  What needs the context or
// a kernel unit's constants -- null context or handle, a handle of another context, workgroup counts, LDS plans -- comes
// after it, in the entry (csrc/mwrt_retrieval.hip).  A call that is not refused allocates nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "../../include/mwrt.h"

namespace mwrt {
namespace records {

// A run of `count` fields of `width` bytes each from offset `begin`: a record is a few of them, ascending.
struct Run { size_t begin, width, count; };
struct Record {
  const char* name;            // "mwrt_oe_step", as the messages spell it
  size_t size;                 // sizeof
  size_t min_size;             // struct_size must reach this ...
  const char* min_what;        // ... "the fixed part (through reserved)"
  Run runs[4];                 // unused ones {0, 0, 0}
};
extern const Record OE_STEP, OE_LM, OE_CHAR, OBS_APPLY, BASIS_APPLY, OBS_WHITEN, OE_NFORM, OE_NFORM_CHAR, OE_SELECT;

// The one cut: *out (rec.size bytes) is the caller's record with every field that is not wholly below
// min(struct_size, rec.size) left zero.  False, *out all zero: struct_size is below rec.min_size.
bool cut(const Record& rec, const void* caller, void* out);

struct Refusal {
  int status = MWRT_OK;
  std::string message;         // empty unless refused
  explicit operator bool() const { return status != MWRT_OK; }
};

enum class LmCall { Prepare, Solve, Cost };      // the three entries of mwrt_oe_lm
enum class CharCall { Gain, Product };           // the two of mwrt_oe_char
enum class WhitenCall { Whiten, Apply };         // the two of mwrt_obs_whiten
enum class NfCall { Prepare, Solve, Cost };      // the three of mwrt_oe_nform
enum class NfCharCall { Char, Gain };            // the two of mwrt_oe_nform_char

Refusal oe_step_args(int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_step* s, mwrt_oe_step* r);
Refusal oe_lm_args(LmCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, mwrt_oe_lm* r);
Refusal oe_char_args(CharCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, mwrt_oe_char* r);
Refusal obs_apply_args(int64_t nprof, int32_t nlev, const mwrt_obs_apply* s, mwrt_obs_apply* r);
// basis_nblk: the blocks of the basis handle
Refusal basis_project_args(int32_t basis_nblk, int64_t nprof, int32_t m, const mwrt_basis_apply* s, mwrt_basis_apply* r);
Refusal basis_expand_args(int64_t nprof, const mwrt_basis_apply* s, mwrt_basis_apply* r);
Refusal whiten_args(WhitenCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* s, mwrt_obs_whiten* r);
// its limit is on n = nblk * nlev (MWRT_OE_NFORM_MAX_N); m is not bounded
Refusal oe_nform_args(NfCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, mwrt_oe_nform* r);
// the same limit; the row window is held to n for Char alone (Gain does not read it)
Refusal oe_nform_char_args(NfCharCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s,
                           mwrt_oe_nform_char* r);
// the same limit; nsel is held to 1 .. m between the reserved field and the pointers
Refusal oe_select_args(int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_select* s, mwrt_oe_select* r);

}  // namespace records
}  // namespace mwrt
