// mwrt_records.cpp -- the argument stage of the record entries (mwrt_records.h says what it covers and in which order).
#include "mwrt_records.h"

#include <cstring>

namespace mwrt {
namespace records {

namespace {
constexpr size_t I32 = sizeof(int32_t), PTR = sizeof(void*);
constexpr const char* FIXED_PART = "the fixed part (through reserved)";

constexpr size_t end_of(const Record& rec) {
  size_t end = 0;
  for (const Run& run : rec.runs) if (run.count) end = run.begin + run.width * run.count;
  return end;
}
}  // namespace

// struct_size and four int32, then pointers to the end
constexpr Record OE_STEP{"mwrt_oe_step", sizeof(mwrt_oe_step), offsetof(mwrt_oe_step, d_status) + PTR,
                         "the required fields (through d_status)", {{0, I32, 5}, {offsetof(mwrt_oe_step, d_k), PTR, 16}}};
constexpr Record OE_LM{"mwrt_oe_lm", sizeof(mwrt_oe_lm), offsetof(mwrt_oe_lm, d_k), FIXED_PART,
                       {{0, I32, 5}, {offsetof(mwrt_oe_lm, d_k), PTR, 25}}};
// ... with four int32 (product .. reserved2) before the last pointer
constexpr Record OE_CHAR{"mwrt_oe_char", sizeof(mwrt_oe_char), offsetof(mwrt_oe_char, d_k), FIXED_PART,
                         {{0, I32, 5}, {offsetof(mwrt_oe_char, d_k), PTR, 19}, {offsetof(mwrt_oe_char, product), I32, 4},
                          {offsetof(mwrt_oe_char, d_out), PTR, 1}}};
constexpr Record OBS_APPLY{"mwrt_obs_apply", sizeof(mwrt_obs_apply), offsetof(mwrt_obs_apply, reserved) + I32, FIXED_PART,
                           {{0, I32, 3}, {offsetof(mwrt_obs_apply, d_tb_in), PTR, 10}}};
constexpr Record BASIS_APPLY{"mwrt_basis_apply", sizeof(mwrt_basis_apply), offsetof(mwrt_basis_apply, reserved) + I32, FIXED_PART,
                             {{0, I32, 2}, {offsetof(mwrt_basis_apply, d_k_in), PTR, 8},
                              {offsetof(mwrt_basis_apply, x_ref_per_profile), I32, 2}}};
// the int64 `reserved` is as wide as the pointers behind it
constexpr Record OBS_WHITEN{"mwrt_obs_whiten", sizeof(mwrt_obs_whiten), offsetof(mwrt_obs_whiten, reserved) + sizeof(int64_t),
                            FIXED_PART, {{0, I32, 4}, {offsetof(mwrt_obs_whiten, reserved), PTR, 17}}};
// struct_size and four int32, then pointers to the end, as mwrt_oe_lm
constexpr Record OE_NFORM{"mwrt_oe_nform", sizeof(mwrt_oe_nform), offsetof(mwrt_oe_nform, d_k), FIXED_PART,
                          {{0, I32, 5}, {offsetof(mwrt_oe_nform, d_k), PTR, 27}}};
// struct_size and five int32, then pointers to the end
constexpr Record OE_NFORM_CHAR{"mwrt_oe_nform_char", sizeof(mwrt_oe_nform_char), offsetof(mwrt_oe_nform_char, d_k), FIXED_PART,
                               {{0, I32, 6}, {offsetof(mwrt_oe_nform_char, d_k), PTR, 18}}};
// struct_size and five int32, then pointers to the end, as mwrt_oe_nform_char
constexpr Record OE_SELECT{"mwrt_oe_select", sizeof(mwrt_oe_select), offsetof(mwrt_oe_select, d_k), FIXED_PART,
                           {{0, I32, 6}, {offsetof(mwrt_oe_select, d_k), PTR, 19}}};
static_assert(end_of(OE_STEP) == sizeof(mwrt_oe_step) && end_of(OE_LM) == sizeof(mwrt_oe_lm) &&
              end_of(OE_CHAR) == sizeof(mwrt_oe_char) && end_of(OBS_APPLY) == sizeof(mwrt_obs_apply) &&
              end_of(BASIS_APPLY) == sizeof(mwrt_basis_apply) && end_of(OBS_WHITEN) == sizeof(mwrt_obs_whiten) &&
              end_of(OE_NFORM) == sizeof(mwrt_oe_nform) && end_of(OE_NFORM_CHAR) == sizeof(mwrt_oe_nform_char) &&
              end_of(OE_SELECT) == sizeof(mwrt_oe_select),
              "the runs of a record end where the record ends");
static_assert(sizeof(int64_t) == PTR, "mwrt_obs_whiten: one run from reserved on");

bool cut(const Record& rec, const void* caller, void* out) {
  std::memset(out, 0, rec.size);
  uint32_t struct_size;
  std::memcpy(&struct_size, caller, sizeof struct_size);
  if (struct_size < rec.min_size) return false;
  const size_t len = struct_size < rec.size ? struct_size : rec.size;
  size_t keep = 0;                                 // the end of the last field wholly below len
  for (const Run& run : rec.runs) {
    if (run.count == 0 || len < run.begin + run.width) break;
    const size_t whole = (len - run.begin) / run.width;
    keep = run.begin + run.width * (whole < run.count ? whole : run.count);
  }
  std::memcpy(out, caller, keep);
  return true;
}

namespace {

Refusal refuse(int status, std::string message) { return Refusal{status, std::move(message)}; }
Refusal invalid(std::string message) { return refuse(MWRT_ERR_INVALID_ARGUMENT, std::move(message)); }
Refusal unsupported(std::string message) { return refuse(MWRT_ERR_UNSUPPORTED, std::move(message)); }

Refusal too_small(const Record& rec) { return invalid(std::string(rec.name) + ".struct_size too small for " + rec.min_what); }
Refusal nlev_limit() { return unsupported("nlev > MWRT_MAX_LEVELS (" + std::to_string(MWRT_MAX_LEVELS) + ")"); }
constexpr int64_t GRID_MAX = 2147483647LL;

inline int32_t reserved_of(const mwrt_oe_step& r) { return r.reserved; }
inline int32_t reserved_of(const mwrt_oe_lm& r) { return r.reserved; }
inline int32_t reserved_of(const mwrt_oe_char& r) { return r.reserved | r.reserved2; }

// The three optimal-estimation records start alike (nblk, xa_per_profile, se_full, reserved, d_k, d_x .. d_fx) and their
// entries check alike; `own(r)` is the entry's part, between the reserved fields and the limits.
template <class R, class Own>
Refusal oe_args(const Record& rec, const char* reserved_what, int64_t nprof, int32_t nlev, int32_t m, const R* s, R* r, Own own) {
  if (!cut(rec, s, r)) return too_small(rec);
  if (nprof < 0 || nlev < 1 || m < 1) return invalid("nprof < 0, nlev < 1 or m < 1");
  if (r->nblk < 1 || r->nblk > 4) return invalid(std::string(rec.name) + ".nblk must be 1 .. 4");
  if (reserved_of(*r) != 0) return invalid(std::string(rec.name) + "." + reserved_what + " must be 0");
  if (Refusal no = own(*r)) return no;
  if (nlev > MWRT_MAX_LEVELS) return nlev_limit();
  if (m > MWRT_OE_MAX_M)
    return unsupported("m > MWRT_OE_MAX_M (" + std::to_string(MWRT_OE_MAX_M) + " observations per profile: G lives in LDS)");
  if (nprof > GRID_MAX) return unsupported("nprof exceeds grid limit");
  return {};
}

template <class R> bool first_blocks(const R& r) {
  bool given = true;
  for (int b = 0; b < r.nblk; ++b) given = given && r.d_k[b];
  return given;
}

// an output that is also one of the inputs
bool whiten_aliased(const mwrt_obs_whiten& r, bool l_is_output) {
  const void* ins[10] = {r.d_se, r.d_y, r.d_fx, r.d_k_in[0], r.d_k_in[1], r.d_k_in[2], r.d_k_in[3],
                         l_is_output ? nullptr : r.d_l, l_is_output ? nullptr : r.d_keep, nullptr};
  const void* outs[9] = {r.d_y_out, r.d_fx_out, r.d_k_out[0], r.d_k_out[1], r.d_k_out[2], r.d_k_out[3],
                         l_is_output ? r.d_l : nullptr, l_is_output ? r.d_keep : nullptr, l_is_output ? r.d_status : nullptr};
  for (const void* o : outs)
    for (const void* i : ins)
      if (o && o == i) return true;
  return false;
}

// what project and expand share
Refusal basis_args(int64_t nprof, const mwrt_basis_apply* s, mwrt_basis_apply* r) {
  if (!cut(BASIS_APPLY, s, r)) return too_small(BASIS_APPLY);
  if (nprof < 0) return invalid("nprof < 0");
  if (r->reserved != 0 || r->reserved2 != 0) return invalid("mwrt_basis_apply.reserved and reserved2 must be 0");
  return {};
}

}  // namespace

Refusal oe_step_args(int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_step* s, mwrt_oe_step* r) {
  return oe_args(OE_STEP, "reserved", nprof, nlev, m, s, r, [](const mwrt_oe_step& r) {
    const bool buffers = r.d_x && r.d_xa && r.d_sa && r.d_se && r.d_y && r.d_fx && r.d_x_new && r.d_status && first_blocks(r);
    return buffers ? Refusal{} : invalid("null buffer");
  });
}

Refusal oe_lm_args(LmCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, mwrt_oe_lm* r) {
  return oe_args(OE_LM, "reserved", nprof, nlev, m, s, r, [call](const mwrt_oe_lm& r) {
    bool buffers = r.d_x && r.d_xa && r.d_se;
    const bool lin = r.d_g0 && r.d_r && r.d_kdx && r.d_keep && r.d_lin_status;
    if (call != LmCall::Cost) buffers = buffers && r.d_sa && lin && first_blocks(r);
    if (call == LmCall::Prepare) buffers = buffers && r.d_y && r.d_fx;
    if (call == LmCall::Solve) buffers = buffers && r.d_gamma && r.d_x_new && r.d_status;
    if (call == LmCall::Cost) buffers = buffers && r.d_y && r.d_fx && r.d_keep && r.d_sa_inv && r.d_cost;
    return buffers ? Refusal{} : invalid("null buffer");
  });
}

Refusal oe_char_args(CharCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, mwrt_oe_char* r) {
  return oe_args(OE_CHAR, "reserved and reserved2", nprof, nlev, m, s, r, [call, nlev](const mwrt_oe_char& r) {
    if (call == CharCall::Gain) {
      if (!(r.d_x && r.d_xa && r.d_sa && r.d_se && r.d_y && r.d_fx && r.d_status && first_blocks(r))) return invalid("null buffer");
      if (!(r.d_gain || r.d_ksa || r.d_keep || r.d_avk_diag || r.d_dfs_block || r.d_noise_var || r.d_smooth_var || r.d_nobs))
        return invalid("mwrt_oe_gain_device: no output asked for beside d_status");
      return Refusal{};
    }
    if (r.product != MWRT_OE_PRODUCT_AVK && r.product != MWRT_OE_PRODUCT_POST_COV)
      return invalid("mwrt_oe_char.product must be MWRT_OE_PRODUCT_AVK or MWRT_OE_PRODUCT_POST_COV");
    bool buffers = r.d_gain && r.d_keep && r.d_out;
    buffers = buffers && (r.product == MWRT_OE_PRODUCT_AVK ? first_blocks(r) : r.d_ksa && r.d_sa);
    if (!buffers) return invalid("null buffer");
    const int64_t n64 = (int64_t)r.nblk * nlev;        // nlev is not yet held to its limit here
    if (r.row_begin < 0 || r.row_count < 0 || (r.row_count == 0 && r.row_begin != 0) || (int64_t)r.row_begin + r.row_count > n64)
      return invalid("mwrt_oe_char: rows row_begin .. row_begin + row_count - 1 must lie in 0 .. n - 1 "
                     "(row_count 0 with row_begin 0: all rows)");
    return Refusal{};
  });
}

Refusal obs_apply_args(int64_t nprof, int32_t nlev, const mwrt_obs_apply* s, mwrt_obs_apply* r) {
  if (!cut(OBS_APPLY, s, r)) return too_small(OBS_APPLY);
  if (nprof < 0 || nlev < 1) return invalid("nprof < 0 or nlev < 1");
  if (r->nblk < 0 || r->nblk > 4) return invalid("mwrt_obs_apply.nblk must be 0 .. 4");
  if (r->reserved != 0) return invalid("mwrt_obs_apply.reserved must be 0");
  if ((r->d_tb_in == nullptr) != (r->d_tb_out == nullptr))
    return invalid("mwrt_obs_apply: d_tb_in and d_tb_out are given together or not at all");
  for (int b = 0; b < r->nblk; ++b)
    if (!r->d_k_in[b] || !r->d_k_out[b]) return invalid("mwrt_obs_apply: null pointer among the first nblk of d_k_in / d_k_out");
  if (!r->d_tb_in && r->nblk == 0) return invalid("mwrt_obs_apply: nothing to do (no TB pair and nblk = 0)");
  bool aliased = r->d_tb_in && r->d_tb_in == r->d_tb_out;
  for (int b = 0; b < r->nblk; ++b) aliased = aliased || r->d_k_in[b] == r->d_k_out[b];
  if (aliased) return invalid("mwrt_obs_apply: an output pointer equals its input (the map is not applied in place)");
  if (nlev > MWRT_MAX_LEVELS) return nlev_limit();
  return {};
}

Refusal basis_project_args(int32_t basis_nblk, int64_t nprof, int32_t m, const mwrt_basis_apply* s, mwrt_basis_apply* r) {
  if (Refusal no = basis_args(nprof, s, r)) return no;
  if (m < 1) return invalid("m < 1");
  for (int b = 0; b < basis_nblk; ++b)
    if (!r->d_k_in[b]) return invalid("mwrt_basis_apply: null pointer among the first nblk of d_k_in");
  if (!r->d_k_out) return invalid("mwrt_basis_apply: d_k_out is null");
  for (int b = 0; b < basis_nblk; ++b)
    if (r->d_k_in[b] == r->d_k_out)
      return invalid("mwrt_basis_apply: d_k_out equals one of its inputs (the product is not formed in place)");
  return {};
}

Refusal basis_expand_args(int64_t nprof, const mwrt_basis_apply* s, mwrt_basis_apply* r) {
  if (Refusal no = basis_args(nprof, s, r)) return no;
  if (!r->d_c || !r->d_x_ref || !r->d_x) return invalid("mwrt_basis_apply: d_c, d_x_ref or d_x is null");
  if (r->d_x == r->d_c || r->d_x == r->d_x_ref)
    return invalid("mwrt_basis_apply: d_x equals one of its inputs (the map is not applied in place)");
  return {};
}

Refusal whiten_args(WhitenCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* s, mwrt_obs_whiten* r) {
  const bool whiten = call == WhitenCall::Whiten;
  if (!cut(OBS_WHITEN, s, r)) return too_small(OBS_WHITEN);
  if (nprof < 0 || nlev < 1 || m < 1) return invalid("nprof < 0, nlev < 1 or m < 1");
  if (r->nblk < 0 || r->nblk > 4) return invalid("mwrt_obs_whiten.nblk must be 0 .. 4");
  if (r->reserved != 0) return invalid("mwrt_obs_whiten.reserved must be 0");
  if (r->mode < 0 || r->mode > (whiten ? 0 : 1))
    return invalid(whiten ? "mwrt_obs_whiten.mode must be 0 in mwrt_obs_whiten_device"
                          : "mwrt_obs_whiten.mode must be 0 (L^-1) or 1 (L^-T)");
  if (whiten) {
    if (!r->d_se || !r->d_y || !r->d_fx || !r->d_l || !r->d_keep || !r->d_status)
      return invalid("mwrt_obs_whiten: d_se, d_y, d_fx, d_l, d_keep or d_status is null");
    for (int b = 0; b < r->nblk; ++b)
      if (!r->d_k_in[b]) return invalid("mwrt_obs_whiten: null pointer among the first nblk of d_k_in");
    if (whiten_aliased(*r, true))
      return invalid("mwrt_obs_whiten: an output pointer equals an input (nothing is whitened in place)");
  } else {
    if (!r->d_l || !r->d_keep) return invalid("mwrt_obs_whiten: d_l or d_keep is null");
    if ((r->d_y == nullptr) != (r->d_y_out == nullptr) || (r->d_fx == nullptr) != (r->d_fx_out == nullptr))
      return invalid("mwrt_obs_whiten: d_y and d_y_out (d_fx and d_fx_out) are given together or not at all");
    for (int b = 0; b < r->nblk; ++b)
      if (!r->d_k_in[b] || !r->d_k_out[b])
        return invalid("mwrt_obs_whiten: null pointer among the first nblk of d_k_in / d_k_out");
    if (!r->d_y && !r->d_fx && r->nblk == 0) return invalid("mwrt_obs_whiten: nothing to do (no vector and nblk = 0)");
    if (whiten_aliased(*r, false))
      return invalid("mwrt_obs_whiten: an output pointer equals an input (nothing is applied in place)");
  }
  if (m > MWRT_OE_MAX_M) return unsupported("m > MWRT_OE_MAX_M (" + std::to_string(MWRT_OE_MAX_M) + ")");
  if (nlev > MWRT_MAX_LEVELS) return nlev_limit();
  return {};
}

// The n-form family: the start of the optimal-estimation records (se_per_profile where they have se_full), the order of
// oe_args, and its own limit -- on n, not on m.
Refusal oe_nform_args(NfCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, mwrt_oe_nform* r) {
  if (!cut(OE_NFORM, s, r)) return too_small(OE_NFORM);
  if (nprof < 0 || nlev < 1 || m < 1) return invalid("nprof < 0, nlev < 1 or m < 1");
  if (r->nblk < 1 || r->nblk > 4) return invalid("mwrt_oe_nform.nblk must be 1 .. 4");
  if (r->reserved != 0) return invalid("mwrt_oe_nform.reserved must be 0");
  bool buffers = r->d_x && r->d_xa;
  if (call == NfCall::Prepare)
    buffers = buffers && r->d_se && r->d_y && r->d_fx && r->d_h && r->d_g && r->d_rwr && r->d_keep && r->d_nobs &&
              r->d_lin_status && first_blocks(*r);
  if (call == NfCall::Solve)
    buffers = buffers && r->d_sa_inv && r->d_h && r->d_g && r->d_rwr && r->d_lin_status && r->d_x_new && r->d_status;
  if (call == NfCall::Cost) buffers = buffers && r->d_sa_inv && r->d_se && r->d_y && r->d_fx && r->d_keep && r->d_cost;
  if (!buffers) return invalid("null buffer");
  if (call == NfCall::Solve && r->d_gamma && (r->d_chi2 || r->d_dfs || r->d_post_var || r->d_post_cov))
    return invalid("mwrt_oe_nform: d_chi2, d_dfs, d_post_var and d_post_cov are defined at gamma = 0 only (d_gamma must be NULL)");
  if ((int64_t)r->nblk * nlev > MWRT_OE_NFORM_MAX_N)
    return unsupported("n = nblk * nlev > MWRT_OE_NFORM_MAX_N (" + std::to_string(MWRT_OE_NFORM_MAX_N) +
                       " state elements per profile: the packed triangle of C lives in LDS)");
  if (nprof > GRID_MAX) return unsupported("nprof exceeds grid limit");
  return {};
}

// The characterisation of the n-form: the order of oe_nform_args with the row window of oe_char_args before the pointers.
Refusal oe_nform_char_args(NfCharCall call, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s,
                           mwrt_oe_nform_char* r) {
  const bool chr = call == NfCharCall::Char;
  if (!cut(OE_NFORM_CHAR, s, r)) return too_small(OE_NFORM_CHAR);
  if (nprof < 0 || nlev < 1 || m < 1) return invalid("nprof < 0, nlev < 1 or m < 1");
  if (r->nblk < 1 || r->nblk > 4) return invalid("mwrt_oe_nform_char.nblk must be 1 .. 4");
  if (r->reserved != 0) return invalid("mwrt_oe_nform_char.reserved must be 0");
  const int64_t n64 = (int64_t)r->nblk * nlev;        // not yet held to its limit here
  if (chr && (r->row_begin < 0 || r->row_count < 0 || (r->row_count == 0 && r->row_begin != 0) ||
              (int64_t)r->row_begin + r->row_count > n64))
    return invalid("mwrt_oe_nform_char: rows row_begin .. row_begin + row_count - 1 must lie in 0 .. n - 1 "
                   "(row_count 0 with row_begin 0: all rows)");
  const bool buffers = chr ? r->d_sa_inv && r->d_h && r->d_lin_status && r->d_status
                           : r->d_se && r->d_keep && r->d_post_cov && r->d_status && r->d_gain && first_blocks(*r);
  if (!buffers) return invalid("null buffer");
  const void* outs[7] = {};
  const void* ins[9] = {};
  if (chr) {
    if (!(r->d_post_cov || r->d_avk || r->d_avk_diag || r->d_noise_var || r->d_smooth_var || r->d_dfs_block))
      return invalid("mwrt_oe_nform_char_device: no output asked for beside d_status");
    const void* o[7] = {r->d_status, r->d_post_cov, r->d_avk, r->d_avk_diag, r->d_noise_var, r->d_smooth_var, r->d_dfs_block};
    const void* i[4] = {r->d_sa_inv, r->d_h, r->d_lin_status, r->d_active};
    for (int k = 0; k < 7; ++k) outs[k] = o[k];
    for (int k = 0; k < 4; ++k) ins[k] = i[k];
  } else {
    outs[0] = r->d_gain;
    const void* i[5] = {r->d_se, r->d_keep, r->d_post_cov, r->d_status, r->d_active};
    for (int k = 0; k < 5; ++k) ins[k] = i[k];
    for (int b = 0; b < r->nblk; ++b) ins[5 + b] = r->d_k[b];
  }
  for (const void* o : outs)
    for (const void* i : ins)
      if (o && o == i) return invalid("mwrt_oe_nform_char: an output pointer equals an input (nothing is formed in place)");
  if (n64 > MWRT_OE_NFORM_MAX_N)
    return unsupported("n = nblk * nlev > MWRT_OE_NFORM_MAX_N (" + std::to_string(MWRT_OE_NFORM_MAX_N) +
                       " state elements per profile: the packed triangles of C and H live in LDS)");
  if (nprof > GRID_MAX) return unsupported("nprof exceeds grid limit");
  return {};
}

// The observation selection: the order of oe_nform_char_args with nsel where that has its row window.
Refusal oe_select_args(int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_select* s, mwrt_oe_select* r) {
  if (!cut(OE_SELECT, s, r)) return too_small(OE_SELECT);
  if (nprof < 0 || nlev < 1 || m < 1) return invalid("nprof < 0, nlev < 1 or m < 1");
  if (r->nblk < 1 || r->nblk > 4) return invalid("mwrt_oe_select.nblk must be 1 .. 4");
  if (r->reserved != 0) return invalid("mwrt_oe_select.reserved must be 0");
  if (r->nsel < 1 || r->nsel > m) return invalid("mwrt_oe_select.nsel must be 1 .. m");
  const bool buffers = r->d_s0 && r->d_se && r->d_order && r->d_q_pick && r->d_rank && r->d_q && r->d_count && r->d_status &&
                       first_blocks(*r);
  if (!buffers) return invalid("null buffer");
  if (r->d_dfs_gain && !r->d_sa_inv)
    return invalid("mwrt_oe_select: d_dfs_gain needs d_sa_inv (the degrees of freedom are taken against the prior)");
  const void* outs[9] = {r->d_order, r->d_q_pick, r->d_rank, r->d_q, r->d_count, r->d_status, r->d_dfs_gain, r->d_post_cov,
                         r->d_post_var};
  const void* ins[10] = {r->d_s0, r->d_se, r->d_sa_inv, r->d_keep, r->d_candidate, r->d_active};
  for (int b = 0; b < r->nblk; ++b) ins[6 + b] = r->d_k[b];
  for (const void* o : outs)
    for (const void* i : ins)
      if (o && o == i) return invalid("mwrt_oe_select: an output pointer equals an input (nothing is formed in place)");
  if ((int64_t)r->nblk * nlev > MWRT_OE_NFORM_MAX_N)
    return unsupported("n = nblk * nlev > MWRT_OE_NFORM_MAX_N (" + std::to_string(MWRT_OE_NFORM_MAX_N) +
                       " state elements per profile: the packed triangle of S lives in LDS)");
  if (nprof > GRID_MAX) return unsupported("nprof exceeds grid limit");
  return {};
}

}  // namespace records
}  // namespace mwrt
