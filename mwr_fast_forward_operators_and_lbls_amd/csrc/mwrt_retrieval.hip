// mwrt_retrieval.hip -- the second host unit of libmwrt.so: the entries that take a versioned record (the optimal-estimation
// step, its Levenberg-Marquardt split and its characterisation, the instrument operator, the reduced-basis state, the
// pre-whitening) and the two handles they use (mwrt_obs, mwrt_basis).  Declarations: include/mwrt.h.
//
// Every entry runs the same stages in the same order: the null / foreign context and handle checks, the argument stage
// (csrc/mwrt_records.h: the record cut at the caller's struct_size, every argument check and the limits of mwrt.h), the
// limits of the launch geometry and the LDS plan, then launch_tail: an empty batch, the device, the stream, the launches.
//
// Host code only: every kernel lives in its own unit (mwrt_oe.hip, mwrt_oe_lm.hip, mwrt_oe_char.hip, mwrt_obs.hip,
// mwrt_basis.hip, mwrt_whiten.hip, mwrt_nform.hip, mwrt_nform_char.hip, mwrt_select.hip) and is reached through the launchers the headers
// below declare.
#include "mwrt_host.hip.h"
#include "mwrt_records.h"
#include "mwrt_oe.hip.h"
#include "mwrt_oe_lm.hip.h"
#include "mwrt_oe_char.hip.h"
#include "mwrt_obs.hip.h"
#include "mwrt_basis.hip.h"
#include "mwrt_whiten.hip.h"
#include "mwrt_nform.hip.h"
#include "mwrt_nform_char.hip.h"
#include "mwrt_select.hip.h"

#include <cmath>
#include <new>

using namespace mwrt;
using records::CharCall;
using records::LmCall;
using records::NfCall;
using records::NfCharCall;
using records::WhitenCall;

struct mwrt_obs : DeviceHandle {    // the blob: w [nnz] | row_ptr [m_out + 1] | col [nnz]
  int32_t m_in = 0, m_out = 0;
  size_t nnz = 0;
};

struct mwrt_basis : DeviceHandle {  // the blob: b [nblk * nlev][r]
  int32_t nblk = 0, nlev = 0, r = 0;
};

namespace {

constexpr int64_t GRID_MAX = 2147483647LL;

int refused(const records::Refusal& no) { return fail(no.status, no.message); }

// ---- the one handle lifecycle ----
// A new H on context c that owns the device copy of host[0 .. bytes).  Synchronous: the blob is in HBM on return.
template <class H> int handle_create(mwrt_context* c, const void* host, size_t bytes, H** out) {
  HIP_TRY(hipSetDevice(c->device));
  H* h = new (std::nothrow) H();
  if (!h) return fail(MWRT_ERR_OUT_OF_MEMORY, "host allocation failed");
  hipError_t e = hipMalloc(&h->d_blob, bytes);
  if (e == hipSuccess) e = hipMemcpy(h->d_blob, host, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (h->d_blob) (void)hipFree(h->d_blob);
    delete h;
    return fail(e == hipErrorOutOfMemory ? MWRT_ERR_OUT_OF_MEMORY : MWRT_ERR_HIP, hipGetErrorString(e));
  }
  h->ctx = c;
  c->handles_live.push_back(h);
  *out = h;
  return MWRT_OK;
}

// While its context lives the blob is freed behind a device-wide drain (launches on any stream may still read it) and the
// handle leaves the context's list; after mwrt_destroy(ctx) only the handle itself is left to delete.
template <class H> int handle_destroy(H* h) {
  if (!h) return MWRT_OK;
  if (mwrt_context* c = h->ctx) {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(h->d_blob);
    for (size_t i = c->handles_live.size(); i-- > 0;)
      if (c->handles_live[i] == h) c->handles_live.erase(c->handles_live.begin() + (long)i);
  }
  delete h;
  return MWRT_OK;
}

// ---- the one launch tail ----
// A launch `fn(st) -> hipError_t` and whether the call wants it.
template <class F> struct Launch { bool wanted; F fn; };
template <class F> Launch<F> launch(F fn) { return {true, fn}; }
template <class F> Launch<F> launch_if(bool wanted, F fn) { return {wanted, fn}; }

// What every record entry ends with: an empty batch is MWRT_OK before the device is touched; else the device, the stream
// and the wanted launches in order, each one timed, up to the first that fails.
template <class... F> int launch_tail(mwrt_context* c, int64_t nprof, void* stream, Launch<F>... launches) {
  if (nprof == 0) return MWRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const hipStream_t st = resolve_stream(c, stream);
  int rc = MWRT_OK;
  ((rc = (rc == MWRT_OK && launches.wanted) ? timed(c, st, [&] { return launches.fn(st); }) : rc), ...);
  return rc;
}

// ---- the optimal-estimation families ----
// What their three records have in common, as the kernels take it.
template <class R> oe::OeArgs oe_kernel_args(const R& r, int32_t nlev, int32_t m) {
  oe::OeArgs o{};
  o.k0 = r.d_k[0]; o.k1 = r.nblk > 1 ? r.d_k[1] : nullptr; o.k2 = r.nblk > 2 ? r.d_k[2] : nullptr;
  o.k3 = r.nblk > 3 ? r.d_k[3] : nullptr;
  o.x = r.d_x; o.xa = r.d_xa; o.sa = r.d_sa; o.se = r.d_se; o.y = r.d_y; o.fx = r.d_fx;
  o.nobs = r.d_nobs; o.status = r.d_status;
  o.nblk = r.nblk; o.nlev = nlev; o.m = m; o.n = r.nblk * nlev;
  o.xa_per_profile = r.xa_per_profile != 0; o.se_full = r.se_full != 0;
  return o;
}

constexpr const char* STEP_LDS = "the optimal-estimation step needs more LDS than this device has per workgroup";
constexpr const char* GAIN_LDS = "the optimal-estimation gain needs more LDS than this device has per workgroup";
constexpr const char* SELECT_LDS = "the observation selection needs more LDS than this device has per workgroup";
int lds_fits(const mwrt_context* c, size_t bytes, const char* or_else) {
  return bytes <= (size_t)c->lds_max ? MWRT_OK : fail(MWRT_ERR_UNSUPPORTED, or_else);
}

// The three entries of the Levenberg-Marquardt split (csrc/mwrt_oe_lm.hip) share one record and differ in the pointers
// they require (the argument stage) and the kernel they launch.
int oe_lm_call(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream, LmCall call) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_oe_lm");
  mwrt_oe_lm r;
  if (const auto no = records::oe_lm_args(call, nprof, nlev, m, s, &r)) return refused(no);
  lm::LmArgs a{};
  a.o = oe_kernel_args(r, nlev, m);
  a.o.x_new = r.d_x_new; a.o.chi2 = r.d_chi2;
  a.gamma = r.d_gamma; a.g0 = r.d_g0; a.r = r.d_r; a.kdx = r.d_kdx; a.keep = r.d_keep; a.lin_status = r.d_lin_status;
  a.active = r.d_active; a.sa_inv = r.d_sa_inv; a.cost = r.d_cost; a.cost_obs = r.d_cost_obs; a.cost_prior = r.d_cost_prior;
  const size_t lds = call == LmCall::Prepare ? oe::lds_plan(m, a.o.n).total_bytes
                   : call == LmCall::Solve ? lm::solve_plan(m, a.o.n).total_bytes
                                           : lm::cost_plan(m, a.o.n, a.o.se_full).total_bytes;
  if (const int rc = lds_fits(c, lds, STEP_LDS)) return rc;
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) {
    return call == LmCall::Prepare ? lm::launch_lm_prepare(a, nprof, st)
         : call == LmCall::Solve ? lm::launch_lm_solve(a, nprof, st)
                                 : lm::launch_lm_cost(a, nprof, st);
  }));
}

// The three entries of the n-form (csrc/mwrt_nform.hip) share one record, too.
int oe_nform_call(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream, NfCall call) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_oe_nform");
  mwrt_oe_nform r;
  if (const auto no = records::oe_nform_args(call, nprof, nlev, m, s, &r)) return refused(no);
  nf::NfArgs a{};
  a.k0 = r.d_k[0]; a.k1 = r.nblk > 1 ? r.d_k[1] : nullptr; a.k2 = r.nblk > 2 ? r.d_k[2] : nullptr;
  a.k3 = r.nblk > 3 ? r.d_k[3] : nullptr;
  a.x = r.d_x; a.xa = r.d_xa; a.sa_inv = r.d_sa_inv; a.se = r.d_se; a.y = r.d_y; a.fx = r.d_fx;
  a.gamma = r.d_gamma; a.active = r.d_active;
  a.h = r.d_h; a.g = r.d_g; a.rwr = r.d_rwr; a.keep = r.d_keep; a.nobs = r.d_nobs; a.lin_status = r.d_lin_status;
  a.x_new = r.d_x_new; a.status = r.d_status;
  a.chi2 = r.d_chi2; a.dfs = r.d_dfs; a.post_var = r.d_post_var; a.post_cov = r.d_post_cov;
  a.cost = r.d_cost; a.cost_obs = r.d_cost_obs; a.cost_prior = r.d_cost_prior;
  a.nblk = r.nblk; a.nlev = nlev; a.m = m; a.n = r.nblk * nlev;
  a.xa_per_profile = r.xa_per_profile != 0; a.se_per_profile = r.se_per_profile != 0;
  const size_t lds = call == NfCall::Prepare ? nf::normal_plan(a.n).total_bytes
                   : call == NfCall::Solve ? nf::solve_plan(a.n).total_bytes
                                           : nf::cost_plan(a.n).total_bytes;
  if (const int rc = lds_fits(c, lds, STEP_LDS)) return rc;
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) {
    return call == NfCall::Prepare ? nf::launch_nf_normal(a, nprof, st)
         : call == NfCall::Solve ? nf::launch_nf_solve(a, nprof, st)
                                 : nf::launch_nf_cost(a, nprof, st);
  }));
}

// The two entries of the n-form's characterisation (csrc/mwrt_nform_char.hip) share one record.
int oe_nform_char_call(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s, void* stream,
                       NfCharCall call) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_oe_nform_char");
  mwrt_oe_nform_char r;
  if (const auto no = records::oe_nform_char_args(call, nprof, nlev, m, s, &r)) return refused(no);
  nfc::CharArgs a{};
  a.k0 = r.d_k[0]; a.k1 = r.nblk > 1 ? r.d_k[1] : nullptr; a.k2 = r.nblk > 2 ? r.d_k[2] : nullptr;
  a.k3 = r.nblk > 3 ? r.d_k[3] : nullptr;
  a.sa_inv = r.d_sa_inv; a.se = r.d_se; a.h = r.d_h; a.lin_status = r.d_lin_status; a.keep = r.d_keep; a.active = r.d_active;
  a.status = r.d_status; a.post_cov = r.d_post_cov; a.avk = r.d_avk; a.avk_diag = r.d_avk_diag; a.noise_var = r.d_noise_var;
  a.smooth_var = r.d_smooth_var; a.dfs_block = r.d_dfs_block; a.gain = r.d_gain;
  a.nblk = r.nblk; a.nlev = nlev; a.m = m; a.n = r.nblk * nlev;
  a.se_per_profile = r.se_per_profile != 0; a.row_begin = r.row_begin; a.rows = r.row_count == 0 ? a.n : r.row_count;
  if (call == NfCharCall::Char) {
    if (const int rc = lds_fits(c, nfc::char_plan(a.n).total_bytes, STEP_LDS)) return rc;
    return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return nfc::launch_nfc_char(a, nprof, st); }));
  }
  // one workgroup per (profile, nfc::ROWS rows, nfc::COLS columns); the column tiles are the grid's second dimension
  if (nprof > GRID_MAX / nfc::gain_row_tiles(m))
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_oe_nform_gain_device: more than 2147483647 workgroups in one launch (split the batch)");
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return nfc::launch_nfc_gain(a, nprof, st); }));
}

// The observation selection (csrc/mwrt_select.hip): one entry, one kernel.
int oe_select_call(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_select* s, void* stream) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_oe_select");
  mwrt_oe_select r;
  if (const auto no = records::oe_select_args(nprof, nlev, m, s, &r)) return refused(no);
  sel::SelArgs a{};
  a.k0 = r.d_k[0]; a.k1 = r.nblk > 1 ? r.d_k[1] : nullptr; a.k2 = r.nblk > 2 ? r.d_k[2] : nullptr;
  a.k3 = r.nblk > 3 ? r.d_k[3] : nullptr;
  a.s0 = r.d_s0; a.se = r.d_se; a.sa_inv = r.d_sa_inv; a.keep = r.d_keep; a.candidate = r.d_candidate; a.active = r.d_active;
  a.order = r.d_order; a.q_pick = r.d_q_pick; a.rank = r.d_rank; a.q = r.d_q; a.count = r.d_count; a.status = r.d_status;
  a.dfs_gain = r.d_dfs_gain; a.post_cov = r.d_post_cov; a.post_var = r.d_post_var;
  a.nblk = r.nblk; a.nlev = nlev; a.m = m; a.n = r.nblk * nlev; a.nsel = r.nsel;
  a.se_per_profile = r.se_per_profile != 0; a.s0_per_profile = r.s0_per_profile != 0;
  if (const int rc = lds_fits(c, sel::sel_plan(a.n).total_bytes, SELECT_LDS)) return rc;
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return sel::launch_select(a, nprof, st); }));
}

// The two entries of the characterisation (csrc/mwrt_oe_char.hip) share one record.
int oe_char_call(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, void* stream, CharCall call) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_oe_char");
  mwrt_oe_char r;
  if (const auto no = records::oe_char_args(call, nprof, nlev, m, s, &r)) return refused(no);
  const oe::OeArgs o = oe_kernel_args(r, nlev, m);
  if (call == CharCall::Gain) {
    oec::GainArgs g{};
    g.o = o;
    g.gain = r.d_gain; g.ksa = r.d_ksa; g.keep = r.d_keep; g.avk_diag = r.d_avk_diag; g.noise_var = r.d_noise_var;
    g.smooth_var = r.d_smooth_var; g.dfs_block = r.d_dfs_block;
    if (const int rc = lds_fits(c, oec::gain_plan(m).total_bytes, GAIN_LDS)) return rc;
    return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return oec::launch_char_gain(g, nprof, st); }));
  }
  oec::ProductArgs a{};
  a.left = r.d_gain; a.keep = r.d_keep; a.out = r.d_out;
  if (r.product == MWRT_OE_PRODUCT_AVK) {
    a.r0 = o.k0; a.r1 = o.k1; a.r2 = o.k2; a.r3 = o.k3;
    a.rcols = nlev;
  } else {
    a.r0 = r.d_ksa; a.rcols = o.n; a.sa = r.d_sa;
  }
  a.m = m; a.n = o.n; a.row_begin = r.row_begin; a.rows = r.row_count == 0 ? o.n : r.row_count;
  a.tiles_x = (o.n + oec::TILE - 1) / oec::TILE; a.tiles_y = (a.rows + oec::TILE - 1) / oec::TILE;
  if ((int64_t)a.tiles_x * a.tiles_y * nprof > GRID_MAX)
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_oe_product_device: more than 2147483647 tiles of 64 x 64 in one call (use row windows)");
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return oec::launch_char_product(a, nprof, st); }));
}

// What the two basis entries check before their argument stage.
int basis_handle(const mwrt_context* c, const mwrt_basis* bs, const mwrt_basis_apply* s) {
  if (!c || !bs || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context, mwrt_basis or mwrt_basis_apply");
  if (bs->ctx != c) return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_basis belongs to another context, or its context was destroyed");
  return MWRT_OK;
}

// the blocks with an output asked for, packed to the front; the vectors as they are
wh::ApplyArgs whiten_apply_args(const mwrt_obs_whiten& r, int32_t nlev, int32_t m) {
  wh::ApplyArgs a{};
  const double* in[4] = {};
  double* out[4] = {};
  int n = 0;
  for (int b = 0; b < r.nblk; ++b)
    if (r.d_k_out[b]) { in[n] = r.d_k_in[b]; out[n] = r.d_k_out[b]; ++n; }
  a.in0 = in[0]; a.in1 = in[1]; a.in2 = in[2]; a.in3 = in[3];
  a.out0 = out[0]; a.out1 = out[1]; a.out2 = out[2]; a.out3 = out[3];
  if (r.d_y_out) { a.v_in0 = r.d_y; a.v_out0 = r.d_y_out; }
  if (r.d_fx_out) { a.v_in1 = r.d_fx; a.v_out1 = r.d_fx_out; }
  a.l = r.d_l; a.keep = r.d_keep;
  a.nblk = n; a.nlev = nlev; a.m = m; a.mode = r.mode;
  a.ctiles = (nlev + wh::COLS - 1) / wh::COLS;
  a.tiles = n * a.ctiles + ((a.v_in0 || a.v_in1) ? 1 : 0);
  return a;
}

// The two entries of the pre-whitening (csrc/mwrt_whiten.hip) share one record; mwrt_obs_whiten_device factorises first.
int whiten_call(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* s, void* stream, WhitenCall call) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_obs_whiten");
  mwrt_obs_whiten r;
  if (const auto no = records::whiten_args(call, nprof, nlev, m, s, &r)) return refused(no);
  // one workgroup per (profile, tile of wh::COLS columns), and one more per profile for the vectors: at most 65 a profile
  const int64_t tiles = (int64_t)r.nblk * ((nlev + wh::COLS - 1) / wh::COLS) + 1;
  if (nprof > GRID_MAX / tiles)
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_obs_whiten: more than 2147483647 workgroups in one launch (split the batch)");
  wh::FactorArgs f{};
  f.k0 = r.d_k_in[0]; f.k1 = r.d_k_in[1]; f.k2 = r.d_k_in[2]; f.k3 = r.d_k_in[3];
  f.se = r.d_se; f.y = r.d_y; f.fx = r.d_fx;
  f.l = r.d_l; f.keep = r.d_keep; f.status = r.d_status;
  f.nblk = r.nblk; f.nlev = nlev; f.m = m; f.se_full = r.se_full != 0;
  const wh::ApplyArgs a = whiten_apply_args(r, nlev, m);
  return launch_tail(c, nprof, stream,
                     launch_if(call == WhitenCall::Whiten, [&](hipStream_t st) { return wh::launch_factor(f, nprof, st); }),
                     launch_if(call == WhitenCall::Apply || a.tiles != 0, [&](hipStream_t st) { return wh::launch_apply(a, nprof, st); }));
}

}  // namespace

extern "C" {

/* The optimal-estimation step (csrc/mwrt_oe.hip). */
size_t mwrt_oe_step_size(void) { return sizeof(mwrt_oe_step); }

int mwrt_oe_step_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_step* s, void* stream) {
  if (!c || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or mwrt_oe_step");
  mwrt_oe_step r;
  if (const auto no = records::oe_step_args(nprof, nlev, m, s, &r)) return refused(no);
  oe::OeArgs a = oe_kernel_args(r, nlev, m);
  a.x_new = r.d_x_new; a.chi2 = r.d_chi2; a.dfs = r.d_dfs; a.post_var = r.d_post_var;
  if (const int rc = lds_fits(c, oe::lds_plan(m, a.n).total_bytes, STEP_LDS)) return rc;
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return oe::launch_oe_step(a, nprof, st); }));
}

/* Its Levenberg-Marquardt split (csrc/mwrt_oe_lm.hip). */
size_t mwrt_oe_lm_size(void) { return sizeof(mwrt_oe_lm); }

int mwrt_oe_lm_prepare_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream) {
  return oe_lm_call(c, nprof, nlev, m, s, stream, LmCall::Prepare);
}
int mwrt_oe_lm_solve_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream) {
  return oe_lm_call(c, nprof, nlev, m, s, stream, LmCall::Solve);
}
int mwrt_oe_cost_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream) {
  return oe_lm_call(c, nprof, nlev, m, s, stream, LmCall::Cost);
}

/* The same step in the n-form (csrc/mwrt_nform.hip). */
size_t mwrt_oe_nform_size(void) { return sizeof(mwrt_oe_nform); }

int mwrt_oe_nform_prepare_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream) {
  return oe_nform_call(c, nprof, nlev, m, s, stream, NfCall::Prepare);
}
int mwrt_oe_nform_solve_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream) {
  return oe_nform_call(c, nprof, nlev, m, s, stream, NfCall::Solve);
}
int mwrt_oe_nform_cost_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream) {
  return oe_nform_call(c, nprof, nlev, m, s, stream, NfCall::Cost);
}

/* The observation selection by information content (csrc/mwrt_select.hip). */
size_t mwrt_oe_select_size(void) { return sizeof(mwrt_oe_select); }

int mwrt_oe_select_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_select* s, void* stream) {
  return oe_select_call(c, nprof, nlev, m, s, stream);
}

/* The characterisation of the n-form step (csrc/mwrt_nform_char.hip). */
size_t mwrt_oe_nform_char_size(void) { return sizeof(mwrt_oe_nform_char); }

int mwrt_oe_nform_char_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s, void* stream) {
  return oe_nform_char_call(c, nprof, nlev, m, s, stream, NfCharCall::Char);
}
int mwrt_oe_nform_gain_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s, void* stream) {
  return oe_nform_char_call(c, nprof, nlev, m, s, stream, NfCharCall::Gain);
}

/* The m-form step's characterisation (csrc/mwrt_oe_char.hip). */
size_t mwrt_oe_char_size(void) { return sizeof(mwrt_oe_char); }

int mwrt_oe_gain_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, void* stream) {
  return oe_char_call(c, nprof, nlev, m, s, stream, CharCall::Gain);
}
int mwrt_oe_product_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, void* stream) {
  return oe_char_call(c, nprof, nlev, m, s, stream, CharCall::Product);
}

/* The instrument operator (csrc/mwrt_obs.hip): a handle that owns the device copy of a CSR map, and its launches. */
uint32_t mwrt_obs_apply_size(void) { return (uint32_t)sizeof(mwrt_obs_apply); }

int mwrt_obs_create(mwrt_context* c, int32_t m_in, int32_t m_out, const int32_t* row_ptr, const int32_t* col, const double* w,
                    mwrt_obs** out) {
  if (out) *out = nullptr;
  if (!c || !row_ptr || !col || !w || !out) return fail(MWRT_ERR_INVALID_ARGUMENT, "null argument");
  if (m_in < 1 || m_out < 1) return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_obs_create: m_in < 1 or m_out < 1");
  if (row_ptr[0] != 0) return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_obs_create: row_ptr[0] must be 0");
  for (int32_t o = 0; o < m_out; ++o)
    if (row_ptr[o + 1] < row_ptr[o])
      return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_obs_create: row_ptr decreases at row " + std::to_string(o));
  const size_t nnz = (size_t)row_ptr[m_out];
  for (size_t e = 0; e < nnz; ++e) {
    if (col[e] < 0 || col[e] >= m_in)
      return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_obs_create: col[" + std::to_string(e) + "] outside 0 .. m_in - 1");
    if (!std::isfinite(w[e]))
      return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_obs_create: w[" + std::to_string(e) + "] is not finite");
  }
  const size_t w_bytes = sizeof(double) * nnz, rp_bytes = sizeof(int32_t) * ((size_t)m_out + 1);
  std::vector<char> host(w_bytes + rp_bytes + sizeof(int32_t) * nnz);
  std::memcpy(host.data(), w, w_bytes);
  std::memcpy(host.data() + w_bytes, row_ptr, rp_bytes);
  std::memcpy(host.data() + w_bytes + rp_bytes, col, sizeof(int32_t) * nnz);
  if (const int rc = handle_create(c, host.data(), host.size(), out)) return rc;
  (*out)->m_in = m_in; (*out)->m_out = m_out; (*out)->nnz = nnz;
  return MWRT_OK;
}

int mwrt_obs_destroy(mwrt_obs* op) { return handle_destroy(op); }

int mwrt_obs_apply_device(mwrt_context* c, const mwrt_obs* op, int64_t nprof, int32_t nlev, const mwrt_obs_apply* s,
                          void* stream) {
  if (!c || !op || !s) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context, mwrt_obs or mwrt_obs_apply");
  if (op->ctx != c) return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_obs belongs to another context, or its context was destroyed");
  mwrt_obs_apply r;
  if (const auto no = records::obs_apply_args(nprof, nlev, s, &r)) return refused(no);
  obs::ObsArgs a{};
  a.w = static_cast<const double*>(op->d_blob);
  a.row_ptr = reinterpret_cast<const int32_t*>(a.w + op->nnz);
  a.col = a.row_ptr + op->m_out + 1;
  a.m_in = op->m_in; a.m_out = op->m_out;
  obs::ObsArgs k = a, t = a;                           // the K blocks at nlev; the TB pair as one block of one level
  k.in0 = r.d_k_in[0]; k.in1 = r.d_k_in[1]; k.in2 = r.d_k_in[2]; k.in3 = r.d_k_in[3];
  k.out0 = r.d_k_out[0]; k.out1 = r.d_k_out[1]; k.out2 = r.d_k_out[2]; k.out3 = r.d_k_out[3];
  k.nlev = nlev; k.nblk = r.nblk; k.nchunks = (nlev + obs::WAVE - 1) / obs::WAVE;
  t.in0 = r.d_tb_in; t.out0 = r.d_tb_out; t.nlev = 1; t.nblk = 1; t.nchunks = 1;
  // one wave per (profile, block, output row, level chunk), ITEMS waves per workgroup; the per-profile count is < 2^37
  const int64_t per_prof = (int64_t)(r.nblk > 0 ? r.nblk : 1) * op->m_out * k.nchunks;
  if (nprof > GRID_MAX * obs::ITEMS / per_prof)
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_obs_apply_device: more than 2147483647 workgroups in one launch (split the batch)");
  k.items = nprof * r.nblk * op->m_out * k.nchunks;
  t.items = nprof * op->m_out;
  return launch_tail(c, nprof, stream,
                     launch_if(r.nblk > 0, [&](hipStream_t st) { return obs::launch_obs_apply(k, st); }),
                     launch_if(r.d_tb_in != nullptr, [&](hipStream_t st) { return obs::launch_obs_apply(t, st); }));
}

/* The reduced-basis state (csrc/mwrt_basis.hip): a handle that owns the device copy of B, and its two launches. */
uint32_t mwrt_basis_apply_size(void) { return (uint32_t)sizeof(mwrt_basis_apply); }

int mwrt_basis_create(mwrt_context* c, int32_t nblk, int32_t nlev, int32_t r, const double* b, mwrt_basis** out) {
  if (out) *out = nullptr;
  if (!c || !b || !out) return fail(MWRT_ERR_INVALID_ARGUMENT, "null argument");
  if (nblk < 1 || nblk > 4) return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_basis_create: nblk must be 1 .. 4");
  if (nlev < 1 || r < 1) return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_basis_create: nlev < 1 or r < 1");
  if (nlev > MWRT_MAX_LEVELS || r > MWRT_MAX_LEVELS)
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_basis_create: nlev or r > MWRT_MAX_LEVELS (" + std::to_string(MWRT_MAX_LEVELS) + ")");
  const size_t count = (size_t)nblk * (size_t)nlev * (size_t)r;
  for (size_t e = 0; e < count; ++e)
    if (!std::isfinite(b[e]))
      return fail(MWRT_ERR_INVALID_ARGUMENT, "mwrt_basis_create: b[" + std::to_string(e / (size_t)r) + "][" +
                                                 std::to_string(e % (size_t)r) + "] is not finite");
  if (const int rc = handle_create(c, b, sizeof(double) * count, out)) return rc;
  (*out)->nblk = nblk; (*out)->nlev = nlev; (*out)->r = r;
  return MWRT_OK;
}

int mwrt_basis_destroy(mwrt_basis* bs) { return handle_destroy(bs); }

int mwrt_basis_project_device(mwrt_context* c, const mwrt_basis* bs, int64_t nprof, int32_t m, const mwrt_basis_apply* s,
                              void* stream) {
  if (const int rc = basis_handle(c, bs, s)) return rc;
  mwrt_basis_apply r;
  if (const auto no = records::basis_project_args(bs->nblk, nprof, m, s, &r)) return refused(no);
  // one workgroup per (ROWS rows, COLS columns): nprof * m rows may fill as many row tiles as the column tiles leave
  const int64_t col_tiles = (bs->r + basis::COLS - 1) / basis::COLS;
  if (nprof > GRID_MAX / col_tiles * basis::ROWS / m)
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_basis_project_device: more than 2147483647 workgroups in one launch (split the batch)");
  basis::ProjectArgs a{};
  a.in0 = r.d_k_in[0]; a.in1 = r.d_k_in[1]; a.in2 = r.d_k_in[2]; a.in3 = r.d_k_in[3];
  a.b = static_cast<const double*>(bs->d_blob); a.out = r.d_k_out;
  a.nrows = nprof * m; a.nlev = bs->nlev; a.nblk = bs->nblk; a.n = bs->nblk * bs->nlev; a.r = bs->r;
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return basis::launch_project(a, st); }));
}

int mwrt_basis_expand_device(mwrt_context* c, const mwrt_basis* bs, int64_t nprof, const mwrt_basis_apply* s, void* stream) {
  if (const int rc = basis_handle(c, bs, s)) return rc;
  mwrt_basis_apply r;
  if (const auto no = records::basis_expand_args(nprof, s, &r)) return refused(no);
  const int64_t n = (int64_t)bs->nblk * bs->nlev;       // <= 4096
  if (nprof > GRID_MAX * basis::THREADS / n)
    return fail(MWRT_ERR_UNSUPPORTED, "mwrt_basis_expand_device: more than 2147483647 workgroups in one launch (split the batch)");
  basis::ExpandArgs a{};
  a.b = static_cast<const double*>(bs->d_blob); a.c = r.d_c; a.x_ref = r.d_x_ref; a.x = r.d_x;
  a.total = nprof * n; a.n = (int32_t)n; a.r = bs->r; a.per_profile = r.x_ref_per_profile != 0;
  return launch_tail(c, nprof, stream, launch([&](hipStream_t st) { return basis::launch_expand(a, st); }));
}

/* Pre-whitening with a per-profile observation-error covariance (csrc/mwrt_whiten.hip): no handle. */
uint32_t mwrt_obs_whiten_size(void) { return (uint32_t)sizeof(mwrt_obs_whiten); }

int mwrt_obs_whiten_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* s, void* stream) {
  return whiten_call(c, nprof, nlev, m, s, stream, WhitenCall::Whiten);
}
int mwrt_obs_whiten_apply_device(mwrt_context* c, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* s,
                                 void* stream) {
  return whiten_call(c, nprof, nlev, m, s, stream, WhitenCall::Apply);
}

}  // extern "C"
