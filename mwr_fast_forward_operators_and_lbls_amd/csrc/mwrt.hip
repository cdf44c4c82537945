// mwrt.hip -- C-ABI host side of libmwrt.so (declarations + reference citations: include/mwrt.h): context and model
// lifecycle, the TB, absorption, layer-optical-depth, Jacobian and parameter-Jacobian entries, and the utilities.  The
// entries that take a versioned record, and the handles they use, are csrc/mwrt_retrieval.hip.
//
// HIP only: there is no CPU fallback in this library.  Without a GPU mwrt_device_count()
// returns 0 and mwrt_create() fails with MWRT_ERR_NO_DEVICE.
//
// Host code only: streams, caches, argument checks and the choice of launch.  Every kernel lives in another unit
// (mwrt_inst.hip, mwrt_tl.hip, mwrt_ray.hip, mwrt_par.hip, mwrt_aux.hip) and is reached through the launchers the headers
// below declare.
#include "mwrt_host.hip.h"
#include "mwrt_args.hip.h"
#include "mwrt_tl.hip.h"
#include "mwrt_ray.hip.h"
#include "mwrt_par.hip.h"
#include "mwrt_plan.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <new>
#include <atomic>

using namespace mwrt;

namespace {
thread_local std::string g_err;
}  // namespace

int mwrt::fail(int code, const std::string& msg) { g_err = msg; return code; }

struct mwrt_model {
  ModelFlat* d_desc = nullptr;
  ModelFlat h_desc;
  uint64_t id = 0;              // process-unique: caches keyed by it survive a destroy / create that reuses the address
};

namespace {

int upload_small(mwrt_context* c, DeviceCache& cache, const double* src, int n, const double** dev) {
  DeviceCache::Blob b;
  const hipError_t e = cache.get(0, 0, src, n, c->stream, [&](std::vector<char>* host) {
    host->assign((const char*)src, (const char*)(src + n));
    return n;
  }, &b);
  HIP_TRY(e);
  *dev = (const double*)b.dev;
  return MWRT_OK;
}

// device copy of chunk_masks(...) for chunks of `nfc` frequencies
int get_masks(mwrt_context* c, const mwrt_model* m, const double* frq, int nf, int nfc, const LineMasks** out) {
  DeviceCache::Blob b;
  const hipError_t e = c->mask_cache.get(m->id, nfc, frq, nf, c->stream, [&](std::vector<char>* host) {
    std::vector<LineMasks> masks;
    chunk_masks(m->h_desc, frq, nf, nfc, &masks);
    host->assign((const char*)masks.data(), (const char*)(masks.data() + masks.size()));
    return (int)masks.size();
  }, &b);
  HIP_TRY(e);
  *out = (const LineMasks*)b.dev;
  return MWRT_OK;
}

// Workspace hand-over between streams (ray-path factors, materialised absorption): stream-ordered, no host wait.
int workspace_acquire(mwrt_context* c, hipStream_t st) {
  if (!c->ws_event) HIP_TRY(hipEventCreateWithFlags(&c->ws_event, hipEventDisableTiming));
  if (c->ws_used && c->ws_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->ws_event, 0));
  return MWRT_OK;
}
int workspace_release(mwrt_context* c, hipStream_t st) {
  HIP_TRY(hipEventRecord(c->ws_event, st));
  c->ws_stream = st; c->ws_used = true;
  return MWRT_OK;
}

// Runs `fn` when the scope is left, whichever return path leaves it (C++17: the guard is never copied).
template <class F> struct ScopeExit {
  F fn;
  ~ScopeExit() { fn(); }
};
template <class F> ScopeExit<F> on_scope_exit(F fn) { return ScopeExit<F>{fn}; }

int check_common(const mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev, int32_t nf) {
  if (!c || !m) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or model");
  if (nprof < 0 || nf < 1) return fail(MWRT_ERR_INVALID_ARGUMENT, "nprof < 0 or nf < 1");
  if (nlev < 2) return fail(MWRT_ERR_INVALID_ARGUMENT, "nlev < 2");
  if (nlev > MWRT_MAX_LEVELS) return fail(MWRT_ERR_UNSUPPORTED, "nlev > MWRT_MAX_LEVELS (one lane per level)");
  if (nprof > 2147483647LL) return fail(MWRT_ERR_UNSUPPORTED, "nprof exceeds grid limit");
  return MWRT_OK;
}

// Grows a workspace that consecutive calls share (never shrinks it): launches queued on any stream may still read
// the old allocation, so the device drains first
hipError_t grow_behind_drain(DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return hipSuccess;
  const hipError_t e = hipDeviceSynchronize();
  return e != hipSuccess ? e : b.reserve(bytes);
}

#if MWRT_PHASE_CLOCK
// diagnostic build: stamps of the LAST launch go to $MWRT_PHASE_DUMP as raw int64 [nprof][4][10] (100-MHz wall clock; slots 8, 9 = HW_ID, XCC_ID)
long long* g_phase = nullptr;
size_t g_phase_cap = 0;
int phase_attach(FusedArgs* a, int64_t nprof, int nchunks, hipStream_t st) {
  const size_t phase_n = (size_t)nprof * 4 * 10;
  a->phase = nullptr;
  if (!std::getenv("MWRT_PHASE_DUMP") || nchunks != 1) return MWRT_OK;
  if (g_phase_cap < phase_n) { if (g_phase) (void)hipFree(g_phase); HIP_TRY(hipMalloc((void**)&g_phase, phase_n * 8)); g_phase_cap = phase_n; }
  HIP_TRY(hipMemsetAsync(g_phase, 0, phase_n * 8, st));
  a->phase = g_phase;
  return MWRT_OK;
}
int phase_dump(const FusedArgs& a, int64_t nprof, hipStream_t st) {
  if (!a.phase) return MWRT_OK;
  const size_t phase_n = (size_t)nprof * 4 * 10;
  std::vector<long long> h(phase_n);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(h.data(), g_phase, phase_n * 8, hipMemcpyDeviceToHost));
  if (FILE* f = std::fopen(std::getenv("MWRT_PHASE_DUMP"), "wb")) { std::fwrite(h.data(), 8, phase_n, f); std::fclose(f); }
  return MWRT_OK;
}
#else
int phase_attach(FusedArgs*, int64_t, int, hipStream_t) { return MWRT_OK; }
int phase_dump(const FusedArgs&, int64_t, hipStream_t) { return MWRT_OK; }
#endif

int launch_fused(mwrt_context* c, int nfc, FusedArgs a, int64_t nprof, hipStream_t st, int variant) {
  int threads = lanes_for(a.nlev);
  // The RTE-from-absorption kernel is light on registers (4 waves per SIMD fit): a fourth wave that holds no
  // level still takes its share of the (frequency, angle, segment) items, 90 serial layer steps instead of 120
  if (variant == FUSED_FROM_ALPHA && threads < 256 && a.nang > 1) threads = 256;
  const int nchunks = (a.nf + nfc - 1) / nfc;
  size_t lds = 0;
  if (!plan_fused(c->lds_max, nfc, a.nlev, a.nf, a.nang, &a.g, &lds, threads))
    return fail(MWRT_ERR_UNSUPPORTED, "LDS budget exceeded (nlev x nang too large)");
  dim3 grid((unsigned)nprof /* = nmodels x profiles */, (unsigned)nchunks), block(threads);
  // valid[] = 1 is written by the kernel itself when one workgroup owns the profile; with several
  // frequency chunks per profile the flags are preset here and the kernel only lowers/raises them
  a.write_valid = nchunks == 1;
  if (!a.write_valid) HIP_TRY(hipMemsetAsync(a.valid, 1, (size_t)nprof, st));
  int rc = phase_attach(&a, nprof, nchunks, st); if (rc) return rc;
  rc = timed(c, st, [&] {
    switch (nfc) {                                    // one translation unit per chunk width (csrc/mwrt_inst.hip)
      case 8: return launch_fused_nfc8(a, grid, block, lds, st, variant);
      case 14: return launch_fused_nfc14(a, grid, block, lds, st, variant);
      default: return launch_fused_nfc16(a, grid, block, lds, st, variant);
    }
  });
  return rc ? rc : phase_dump(a, nprof, st);
}

int launch_absorb(mwrt_context* c, int nfc, const AbsorbArgs& a, int64_t nprof, hipStream_t st) {
  const int nchunks = (a.nf + nfc - 1) / nfc;
  dim3 grid((unsigned)nprof, (unsigned)nchunks), block(lanes_for(a.nlev));
  return timed(c, st, [&] {
    switch (nfc) {
      case 8: return launch_absorb_nfc8(a, grid, block, st);
      case 14: return launch_absorb_nfc14(a, grid, block, st);
      default: return launch_absorb_nfc16(a, grid, block, st);
    }
  });
}

// the windowed absorption kernel on a list absorption_route() gave it: absorption coefficients, or with `T` the layer
// optical depths.  Its tables are the device copy of build_windows(...) in pack_windows' layout and the WIN_NFC masks.
int launch_windowed_absorption(mwrt_context* c, const mwrt_model* m, int64_t nprof, int nlev, const double* d_p, const double* d_t,
                               const double* d_rh, int nf, const double* frq, const double* dev_frq, double* d_awet,
                               double* d_adry, const TauOut* T, int threads, hipStream_t st) {
  DeviceCache::Blob b;
  const hipError_t e = c->win_cache.get(m->id, 0, frq, nf, c->stream, [&](std::vector<char>* host) {
    WindowSet ws;
    build_windows(m->h_desc, frq, nf, &ws);
    pack_windows(ws, nf, host);
    return (int)ws.wins.size();
  }, &b);
  HIP_TRY(e);
  const WindowLayout l = window_layout(b.count, nf);
  AbsorbWinArgs w{};
  w.M = m->d_desc; w.p = d_p; w.t = d_t; w.rh = d_rh; w.frq = dev_frq;
  w.win = (const WinDesc*)b.dev; w.lagrange = (const double*)(b.dev + l.off_lag);
  w.lagrange_h = (const double*)(b.dev + l.off_lagh); w.lag_sd = (const double*)(b.dev + l.off_lagsd);
  int rc = get_masks(c, m, frq, nf, WIN_NFC, &w.masks); if (rc) return rc;
  w.awet = d_awet; w.adry = d_adry; w.nlev = nlev; w.nf = nf;
  if (T) w.T = *T;
  return timed(c, st, [&] { return launch_absorb_win(w, dim3((unsigned)nprof, (unsigned)b.count), dim3(threads), st, T != nullptr); });
}

// K1 (+ layer step): d_tau [nprof][nlev][fpitch], d_valid [nprof].  Windowed kernel when the list qualifies
// (and the mode allows), else every line at every frequency.
int layer_tau_launch(mwrt_context* c, const mwrt_model* m, int64_t nprof, int nlev, const double* d_z, const double* d_p,
                     const double* d_t, const double* d_rh, int nf, const double* frq, const double* dev_frq,
                     double* d_tau, int fpitch, uint8_t* d_valid, hipStream_t st) {
  const int threads = tau_threads(nlev);
  if (threads > 1024) return fail(MWRT_ERR_UNSUPPORTED, "layer optical depths: nlev > 1009");
  const AbsorbRoute route = absorption_route(c->absorption_mode, c->lds_max, frq, nf, threads);
  if (route == AbsorbRoute::refused)
    return fail(MWRT_ERR_UNSUPPORTED, "windowed absorption needs >= 128 strictly increasing frequencies in windows <= 6 GHz wide, "
                                      "<= 505 levels");
  HIP_TRY(hipMemsetAsync(d_valid, 1, (size_t)nprof, st));
  const TauOut T{d_z, d_tau, d_valid, fpitch};
  if (route == AbsorbRoute::windowed)
    return launch_windowed_absorption(c, m, nprof, nlev, d_p, d_t, d_rh, nf, frq, dev_frq, nullptr, nullptr, &T, threads, st);
  AbsorbArgs a{};
  a.M = m->d_desc; a.p = d_p; a.t = d_t; a.rh = d_rh; a.frq = dev_frq; a.nlev = nlev; a.nf = nf; a.T = T;
  { int rc = get_masks(c, m, frq, nf, TAU_NFC, &a.masks); if (rc) return rc; }
  return timed(c, st, [&] {
    return launch_absorb_tau(a, dim3((unsigned)nprof, (unsigned)((nf + TAU_NFC - 1) / TAU_NFC)), dim3(threads), st);
  });
}

// K2: TBs from layer optical depths; the elevations go through in groups of <= 8 (or 10) per launch
int rte_tau_launch(mwrt_context* c, const mwrt_model* m, int64_t nprof, int nlev, const double* d_tau, int fpitch,
                   const double* d_t, int nf, const double* dev_frq, int nang, const double* dev_am, double* d_tb,
                   const uint8_t* d_valid, hipStream_t st) {
  RteTauArgs r{};
  r.M = m->d_desc; r.tau = d_tau; r.t = d_t; r.frq = dev_frq; r.airmass = dev_am; r.tb = d_tb; r.valid = d_valid;
  r.nlev = nlev; r.nf = nf; r.nang = nang; r.fpitch = fpitch;
  const dim3 grid((unsigned)nprof, (unsigned)((nf + RTE_THREADS - 1) / RTE_THREADS));
  const size_t lds = sizeof(double) * 2 * (size_t)nlev;
  for (int a0 = 0; a0 < nang;) {
    const int na = rte_tau_angles(nang - a0);
    r.a0 = a0;
    const int rc = timed(c, st, [&] { return launch_rte_tau(r, grid, lds, st, na); });
    if (rc) return rc;
    a0 += na;
  }
  return MWRT_OK;
}

// ---- the preamble the entry points share ----
// An entry's own check, evaluated by the entry and reported in its place among the shared ones (the tests pin which
// status comes out when several checks would fire)
struct Check { int code; const char* msg; };
constexpr Check PASS{MWRT_OK, nullptr};

enum : unsigned {
  CALL_ANGLES = 1,       // the entry takes elevations: nang is range-checked, the air masses are uploaded
  CALL_HOST = 2,         // host-buffer entry: the context's own stream; nprof == 0 returns before hipSetDevice, not after
  CALL_STAGES = 4,       // ... that hands its staged buffers to a device entry: no NaN check and no uploads of its own
  CALL_NAN_BLANKS = 8    // tb_launch: a NaN frequency or all-NaN elevations is reported in Call::blank instead of failing
};

struct CallSpec {
  unsigned flags;
  int64_t nprof; int nlev, nf; const double* frq;
  int nang; const double* elev;            // (0, nullptr without CALL_ANGLES)
  void* stream;                            // the entry's `stream` argument (device entries)
  bool buffers_ok;                         // every pointer argument the entry requires is given
  Check after_common = PASS, after_buffers = PASS, before_device = PASS;
};

struct Call {
  hipStream_t st = nullptr;
  const double* dev_frq = nullptr;
  const double* dev_am = nullptr;
  bool empty = false;                      // nprof == 0: nothing to do
  bool blank = false;                      // CALL_NAN_BLANKS
};

int begin_call(mwrt_context* c, const mwrt_model* const* ms, int nmodels, const CallSpec& s, Call* call) {
  for (int i = 0; i < nmodels; ++i) {
    int rc = check_common(c, ms[i], s.nprof, s.nlev, s.nf);
    if (rc) return rc;
  }
  if (s.after_common.code) return fail(s.after_common.code, s.after_common.msg);
  const bool angles = s.flags & CALL_ANGLES, stages = s.flags & CALL_STAGES, blanks = s.flags & CALL_NAN_BLANKS;
  if (angles && (s.nang < 1 || s.nang > MWRT_MAX_ANGLES)) return fail(MWRT_ERR_INVALID_ARGUMENT, "nang out of range");
  if (!s.buffers_ok) return fail(MWRT_ERR_INVALID_ARGUMENT, "null buffer");
  if (s.after_buffers.code) return fail(s.after_buffers.code, s.after_buffers.msg);
  if (!stages && !blanks && any_nan(s.frq, s.nf)) return fail(MWRT_ERR_INVALID_ARGUMENT, "NaN frequency");
  if (s.before_device.code) return fail(s.before_device.code, s.before_device.msg);
  call->empty = s.nprof == 0;
  if ((s.flags & CALL_HOST) && call->empty) return MWRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  call->st = (s.flags & CALL_HOST) ? c->stream : resolve_stream(c, s.stream);
  if (call->empty || stages) return MWRT_OK;
  // check_for_nans covers frqs and ang too (PyRTlib_processing.py:77-78): a NaN frequency (the
  // wrapper's frqs array is shared by every call) leaves everything NaN, valid = 0
  call->blank = blanks && (any_nan(s.frq, s.nf) || all_nan(s.elev, s.nang));
  if (call->blank) return MWRT_OK;
  if (angles) {
    std::vector<double> am;
    if (!airmass_of(s.elev, s.nang, &am)) return fail(MWRT_ERR_INVALID_ARGUMENT, "elevation angles must lie in (0, 180) degrees");
    int rc = upload_small(c, c->frq_cache, s.frq, s.nf, &call->dev_frq); if (rc) return rc;
    return upload_small(c, c->am_cache, am.data(), s.nang, &call->dev_am);
  }
  return upload_small(c, c->frq_cache, s.frq, s.nf, &call->dev_frq);
}

// The seven optional output columns (mwrt_tb_extras): taulay holds a value per (frequency, level), the others per
// (elevation, frequency)
struct ExtraSlot {
  double* mwrt_tb_extras::*col;
  bool per_level;
  size_t row(int nlev, int nf, int nang) const { return per_level ? (size_t)nf * nlev : (size_t)nang * nf; }   // doubles per profile
};
constexpr ExtraSlot EXTRA_SLOTS[] = {{&mwrt_tb_extras::tbatm, false},  {&mwrt_tb_extras::tmr, false},    {&mwrt_tb_extras::tauwet, false},
                                     {&mwrt_tb_extras::taudry, false}, {&mwrt_tb_extras::taulay, true},  {&mwrt_tb_extras::tauliq, false},
                                     {&mwrt_tb_extras::tauice, false}};
constexpr int NEX = sizeof(EXTRA_SLOTS) / sizeof(EXTRA_SLOTS[0]);

// host-buffer entries: the k input arrays of `n` doubles each, side by side in d_in
int stage_in(mwrt_context* c, hipStream_t st, size_t n, const double* const* src, int k) {
  HIP_TRY(c->d_in.reserve((size_t)k * n * sizeof(double)));
  for (int i = 0; i < k; ++i)
    HIP_TRY(hipMemcpyAsync(c->d_in.as<double>() + (size_t)i * n, src[i], n * sizeof(double), hipMemcpyHostToDevice, st));
  return MWRT_OK;
}

// The device K-matrix behind its entries (clear, cloud, retrieval variables, ray paths): k_absorb_tl into the context's
// workspace, then k_jac_rte.  `ddz_required`: the entries without mwrt_jac_variables have no optional thickness row.
// `ray`: the ray-traced entry -- options->ray_tracing is not consulted, ray::k_ray_paths_tl fills the context's path
// workspace first and ray::k_jac_rte_ray takes the place of k_jac_rte.
int jacobian_vars_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                         const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                         int32_t nf, const double* frq, int32_t nang, const double* elev,
                         double* d_tb, double* d_dtb_dt, double* d_dtb_dh, double* d_dtb_ddz,
                         double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                         const mwrt_tb_options* opt, const mwrt_jac_variables* vars, bool ddz_required, bool ray, void* stream) {
  const double* d_denliq = opt ? opt->denliq : nullptr;
  const double* d_denice = opt ? opt->denice : nullptr;
  CallSpec s{CALL_ANGLES, nprof, nlev, nf, frq, nang, elev, stream};
  if (!ray && opt && opt->ray_tracing != 0) s.after_common = Check{MWRT_ERR_UNSUPPORTED, "the K-matrix is plane-parallel: ray_tracing is not supported"};
  else if (opt && opt->o3n) s.after_common = Check{MWRT_ERR_UNSUPPORTED, "the K-matrix has no ozone tangent: o3n is not supported"};
  else if (d_dtb_dliq && !d_denliq) s.after_common = Check{MWRT_ERR_INVALID_ARGUMENT, "d_dtb_dliq given without options->denliq"};
  else if (d_dtb_dice && !d_denice) s.after_common = Check{MWRT_ERR_INVALID_ARGUMENT, "d_dtb_dice given without options->denice"};
  else if (vars && (vars->humidity < 0 || vars->humidity > 2 || vars->cloud < 0 || vars->cloud > 1 || vars->heights < 0 ||
                    vars->heights > 1 || vars->reserved != 0))
    s.after_common = Check{MWRT_ERR_INVALID_ARGUMENT, "mwrt_jac_variables: a mode out of range, or reserved != 0"};
  s.buffers_ok = d_z && d_p && d_t && d_rh && frq && elev && d_tb && d_dtb_dt && d_dtb_dh && (d_dtb_ddz || !ddz_required) && d_valid;
  if (nprof * nf > 2147483647LL) s.before_device = Check{MWRT_ERR_UNSUPPORTED, "nprof x nf exceeds grid limit"};
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  hipStream_t st = call.st;
  const double *dev_frq = call.dev_frq, *dev_am = call.dev_am;
  const size_t nabs = (size_t)nprof * nf * nlev;
  HIP_TRY(grow_behind_drain(c->d_jac, sizeof(double) * 6 * nabs + sizeof(unsigned) * (size_t)nprof));
  const double* dev_elev = nullptr;
  if (ray) {
    // the path workspace of the forward's ray tracing, six rows per (profile, elevation) instead of one (grown only)
    rc = upload_small(c, c->elev_cache, elev, nang, &dev_elev); if (rc) return rc;
    HIP_TRY(grow_behind_drain(c->d_amf, sizeof(double) * ray::PATH_ROWS * (size_t)nprof * nang * nlev));
    HIP_TRY(grow_behind_drain(c->d_duct, (size_t)nprof));
  }
  rc = workspace_acquire(c, st); if (rc) return rc;
  auto handover = on_scope_exit([&] { (void)workspace_release(c, st); });    // on every return path from here on
  double* w = c->d_jac.as<double>();
  unsigned* flags = reinterpret_cast<unsigned*>(w + 6 * nabs);
  HIP_TRY(hipMemsetAsync(flags, 0, sizeof(unsigned) * (size_t)nprof, st));
  if (ray) {
    HIP_TRY(hipMemsetAsync(c->d_duct.p, 0, (size_t)nprof, st));
    ray::PathTlArgs pa{};
    pa.z = d_z; pa.p = d_p; pa.t = d_t; pa.rh = d_rh; pa.elev_deg = dev_elev;
    pa.path = c->d_amf.as<double>(); pa.duct = c->d_duct.as<uint8_t>(); pa.nlev = nlev; pa.nang = nang;
    rc = timed(c, st, [&] { return ray::launch_ray_paths_tl(pa, nprof, st); });
    if (rc) return rc;
  }
  AbsorbTlArgs ta{};
  ta.M = m->d_desc; ta.p = d_p; ta.t = d_t; ta.rh = d_rh; ta.frq = dev_frq;
  ta.awet = w; ta.adry = w + nabs; ta.dawet_dt = w + 2 * nabs; ta.dawet_de = w + 3 * nabs;
  ta.dadry_dt = w + 4 * nabs; ta.dadry_de = w + 5 * nabs;
  ta.flags = flags; ta.nlev = nlev; ta.nf = nf; ta.nslab = (nlev + WAVE - 1) / WAVE;
  rc = timed(c, st, [&] { return launch_absorb_tl(ta, nprof, st); });
  if (rc) return rc;
  JacRteArgs ja{};
  ja.M = m->d_desc; ja.z = d_z; ja.t = d_t;
  ja.awet = ta.awet; ja.adry = ta.adry; ja.dawet_dt = ta.dawet_dt; ja.dawet_de = ta.dawet_de;
  ja.dadry_dt = ta.dadry_dt; ja.dadry_de = ta.dadry_de; ja.flags = flags;
  ja.frq = dev_frq; ja.airmass = dev_am;
  ja.tb = d_tb; ja.dtb_dt = d_dtb_dt; ja.dtb_de = d_dtb_dh; ja.dtb_ddz = d_dtb_ddz; ja.valid = d_valid;
  ja.nlev = nlev; ja.nf = nf; ja.nang = nang;
  ja.denliq = d_denliq; ja.denice = d_denice; ja.dtb_dliq = d_dtb_dliq; ja.dtb_dice = d_dtb_dice;
  ja.p = d_p; ja.rh = d_rh;
  if (vars) { ja.humidity = vars->humidity; ja.cloud = vars->cloud; ja.heights = vars->heights; }
  // with cloud arrays the kernel only lowers valid (k_jac_rte): preset it
  if (d_denliq || d_denice) HIP_TRY(hipMemsetAsync(d_valid, 1, (size_t)nprof, st));
  if (ray) {
    const ray::RayRteArgs ra{ja, c->d_amf.as<double>(), c->d_duct.as<uint8_t>()};
    return timed(c, st, [&] { return ray::launch_jac_rte_ray(ra, nprof, st); });
  }
  return timed(c, st, [&] { return launch_jac_rte(ja, nprof, st); });
}

// ... and behind its two HOST-buffer entries, synchronous: staged through device buffers of this call's own (freed on
// every return path), one jacobian_vars_device call on the context's stream -- which makes every check and every
// decision (valid, NaN rows) -- and the results copied back as they are.
int jacobian_vars_host(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                       const double* z, const double* p, const double* t, const double* rh,
                       int32_t nf, const double* frq, int32_t nang, const double* elev,
                       double* tb, double* dtb_dt, double* dtb_dh, double* dtb_ddz, double* dtb_dliq, double* dtb_dice,
                       uint8_t* valid, const mwrt_tb_options* opt, const mwrt_jac_variables* vars, bool ddz_required, bool ray) {
  CallSpec s{CALL_ANGLES | CALL_HOST | CALL_STAGES, nprof, nlev, nf, frq, nang, elev, nullptr};
  s.buffers_ok = z && p && t && rh && frq && elev && tb && dtb_dt && dtb_dh && (dtb_ddz || !ddz_required) && valid;
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  hipStream_t st = call.st;
  const size_t nin = (size_t)nprof * nlev, ntb = (size_t)nprof * nang * nf, njac = ntb * nlev;
  const double* in[6] = {z, p, t, rh, opt ? opt->denliq : nullptr, opt ? opt->denice : nullptr};
  double* out[5] = {dtb_dt, dtb_dh, dtb_ddz, dtb_dliq, dtb_dice};
  size_t nsrc = 0, nrows = 0;
  for (const double* x : in) nsrc += x != nullptr;
  for (const double* x : out) nrows += x != nullptr;
  DevBuf buf;                                                     // this call's own: inputs | tb | rows | valid
  auto free_buf = on_scope_exit([&] { buf.release(); });
  HIP_TRY(buf.reserve(sizeof(double) * (nsrc * nin + ntb + nrows * njac) + (size_t)nprof));
  double* q = buf.as<double>();
  const double* din[6] = {};
  for (int k = 0; k < 6; ++k)
    if (in[k]) {
      HIP_TRY(hipMemcpyAsync(q, in[k], sizeof(double) * nin, hipMemcpyHostToDevice, st));
      din[k] = q; q += nin;
    }
  double* d_tb = q; q += ntb;
  double* dout[5] = {};
  for (int k = 0; k < 5; ++k) if (out[k]) { dout[k] = q; q += njac; }
  uint8_t* d_valid = reinterpret_cast<uint8_t*>(q);
  mwrt_tb_options dopt{};
  if (opt) { dopt = *opt; dopt.denliq = din[4]; dopt.denice = din[5]; }
  rc = jacobian_vars_device(c, m, nprof, nlev, din[0], din[1], din[2], din[3], nf, frq, nang, elev, d_tb, dout[0], dout[1],
                            dout[2], dout[3], dout[4], d_valid, opt ? &dopt : nullptr, vars, ddz_required, ray, nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(tb, d_tb, sizeof(double) * ntb, hipMemcpyDeviceToHost, st));
  for (int k = 0; k < 5; ++k)
    if (out[k]) HIP_TRY(hipMemcpyAsync(out[k], dout[k], sizeof(double) * njac, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(valid, d_valid, (size_t)nprof, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MWRT_OK;
}

}  // namespace

extern "C" {

int mwrt_version(void) { return MWRT_VERSION; }

size_t mwrt_model_desc_size(void) { return sizeof(mwrt_model_desc); }

int mwrt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

const char* mwrt_last_error(void) { return g_err.c_str(); }

int mwrt_create(int device_id, mwrt_context** out) {
  if (!out) return fail(MWRT_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  const int n = mwrt_device_count();
  if (n <= 0) return fail(MWRT_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device_id < 0 || device_id >= n) return fail(MWRT_ERR_INVALID_ARGUMENT, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  mwrt_context* c = new (std::nothrow) mwrt_context();
  if (!c) return fail(MWRT_ERR_OUT_OF_MEMORY, "host allocation failed");
  c->device = device_id;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return fail(MWRT_ERR_HIP, hipGetErrorString(e)); }
  int lds = 0;
  if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && lds > 0)
    c->lds_max = lds;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->num_cus = cus;
  if (const char* mb = std::getenv("MWRT_ALPHA_BATCH_MB")) {       // diagnostic: size of a fine-grid profile batch
    const long v = std::atol(mb);
    if (v > 0) c->alpha_batch_bytes = (size_t)v << 20;
  }
  *out = c;
  return MWRT_OK;
}

int mwrt_destroy(mwrt_context* c) {
  if (!c) return MWRT_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->win_cache.release(); c->mask_cache.release();
  c->frq_cache.release(); c->am_cache.release(); c->elev_cache.release(); c->d_amf.release(); c->d_duct.release(); c->d_alpha.release();
  c->d_jac.release();
  c->d_par.release(); c->par_cache.release();
  c->d_in.release(); c->d_out.release();
  c->d_valid.release(); c->d_ex.release();
  for (DeviceHandle* h : c->handles_live) {             // the handles stay valid for their *_destroy; every entry refuses them
    (void)hipFree(h->d_blob);
    h->d_blob = nullptr; h->ctx = nullptr;
  }
  for (hipEvent_t e : c->ev0) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev1) (void)hipEventDestroy(e);
  if (c->ws_event) (void)hipEventDestroy(c->ws_event);
  (void)hipStreamDestroy(c->stream);
  delete c;
  return MWRT_OK;
}

int mwrt_model_create(mwrt_context* c, const mwrt_model_desc* desc, mwrt_model** out) {
  if (!c || !desc || !out) return fail(MWRT_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (desc->n_h2o < 0 || desc->n_h2o > MWRT_MAX_H2O_LINES || desc->n_o2 < 0 || desc->n_o2 > MWRT_MAX_O2_LINES)
    return fail(MWRT_ERR_INVALID_ARGUMENT, "line counts out of range");
  if (desc->n_x < 0 || desc->n_x > MWRT_MAX_X_LINES) return fail(MWRT_ERR_INVALID_ARGUMENT, "extra-species line count out of range");
  HIP_TRY(hipSetDevice(c->device));
  mwrt_model* m = new (std::nothrow) mwrt_model();
  if (!m) return fail(MWRT_ERR_OUT_OF_MEMORY, "host allocation failed");
  static std::atomic<uint64_t> next_id{1};
  m->id = next_id.fetch_add(1);
  static_cast<mwrt_model_desc&>(m->h_desc) = *desc;
  std::memset(m->h_desc.o2r, 0, sizeof(m->h_desc.o2r));
  std::memset(m->h_desc.h2or, 0, sizeof(m->h_desc.h2or));
  for (int k = 0; k < MWRT_MAX_O2_LINES; ++k) {
    const double rf2 = (k < desc->n_o2 && desc->o2_f[k] != 0.0) ? 1.0 / (desc->o2_f[k] * desc->o2_f[k]) : 0.0;
    m->h_desc.o2_rf2[k] = rf2;
    O2Rec& r = m->h_desc.o2r[k];
    r.f = desc->o2_f[k]; r.s300rf2 = desc->o2_s300[k] * rf2; r.be = desc->o2_be[k]; r.w300 = desc->o2_w300[k];
    r.y0 = desc->o2_y0[k]; r.y1 = desc->o2_y1[k]; r.g0 = desc->o2_g0[k]; r.g1 = desc->o2_g1[k];
    r.dnu0 = desc->o2_dnu0[k]; r.dnu1 = desc->o2_dnu1[k];
  }
  for (int k = 0; k < MWRT_MAX_H2O_LINES; ++k) {
    H2ORec& r = m->h_desc.h2or[k];
    const double fl = desc->h2o_fl[k];
    r.fl = fl; r.s1 = (k < desc->n_h2o && fl != 0.0) ? desc->h2o_s1[k] / (fl * fl) : 0.0; r.b2 = desc->h2o_b2[k];
    r.w0 = desc->h2o_w0[k]; r.x = desc->h2o_x[k]; r.w0s = desc->h2o_w0s[k]; r.xs = desc->h2o_xs[k];
    r.sh = desc->h2o_sh[k]; r.xh = desc->h2o_xh[k]; r.shs = desc->h2o_shs[k]; r.xhs = desc->h2o_xhs[k];
    r.aair = desc->h2o_aair[k]; r.aself = desc->h2o_aself[k]; r.w2 = desc->h2o_w2[k];
  }
  hipError_t e = hipMalloc((void**)&m->d_desc, sizeof(ModelFlat));
  if (e == hipSuccess) e = hipMemcpy(m->d_desc, &m->h_desc, sizeof(ModelFlat), hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (m->d_desc) (void)hipFree(m->d_desc); delete m; return fail(MWRT_ERR_HIP, hipGetErrorString(e)); }
  *out = m;
  return MWRT_OK;
}

int mwrt_model_destroy(mwrt_context* c, mwrt_model* m) {
  if (!m) return MWRT_OK;
  if (c) {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();                       // launches on any stream may still read the tables / windows
    c->win_cache.drop_model(m->id);                     // window descriptors and masks are keyed by the model: drop this one's
    c->mask_cache.drop_model(m->id);
  }
  if (m->d_desc) (void)hipFree(m->d_desc);
  delete m;
  return MWRT_OK;
}

// core of every TB entry point: nmodels absorption models x nprof profiles in ONE launch
static int tb_launch(mwrt_context* c, int nmodels, const mwrt_model* const* ms, int64_t nprof, int32_t nlev,
                     const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                     int32_t nf, const double* frq, int32_t nang, const double* elev,
                     double* d_tb, uint8_t* d_valid, const mwrt_tb_extras* ex, void* stream,
                     const mwrt_tb_options* opt = nullptr, const double* d_awet = nullptr, const double* d_adry = nullptr) {
  if (nmodels < 1 || nmodels > MAX_MULTI || !ms) return fail(MWRT_ERR_INVALID_ARGUMENT, "nmodels must be 1..8");
  const bool cloudy = opt && (opt->denliq || opt->denice);
  const bool rays = opt && opt->ray_tracing != 0;
  const bool ozone = opt && opt->o3n;
  const bool use_opt = cloudy || rays || ozone;
  if (ozone)
    for (int i = 0; i < nmodels; ++i)
      if (ms[i] && ms[i]->h_desc.n_x <= 0)
        return fail(MWRT_ERR_UNSUPPORTED, "o3n given but the model carries no extra-species line table (mwrt_model_desc.n_x = 0)");
  const bool from_alpha = d_awet != nullptr;
  const int64_t rows = nprof * nmodels;
  CallSpec s{CALL_ANGLES | CALL_NAN_BLANKS, nprof, nlev, nf, frq, nang, elev, stream};
  s.buffers_ok = d_z && d_t && frq && elev && d_tb && d_valid && (from_alpha ? d_adry != nullptr : d_p && d_rh);
  if (rows > 2147483647LL) s.after_buffers = Check{MWRT_ERR_UNSUPPORTED, "nmodels x nprof exceeds grid limit"};
  Call call;
  int rc = begin_call(c, ms, nmodels, s, &call);
  if (rc || call.empty) return rc;
  hipStream_t st = call.st;
  if (call.blank) {                                   // the one place where NaN inputs blank the outputs instead of failing
    HIP_TRY(hipMemsetAsync(d_tb, 0xFF, (size_t)rows * nang * nf * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(d_valid, 0, (size_t)rows, st));
    for (const ExtraSlot& x : EXTRA_SLOTS)
      if (ex && ex->*x.col) HIP_TRY(hipMemsetAsync(ex->*x.col, 0xFF, (size_t)rows * x.row(nlev, nf, nang) * sizeof(double), st));
    return MWRT_OK;
  }
  const double *dev_frq = call.dev_frq, *dev_am = call.dev_am;

  FusedArgs a{};
  for (int i = 0; i < nmodels; ++i) a.Ms[i] = ms[i]->d_desc;
  a.nprof_in = nprof;
  a.z = d_z; a.p = d_p; a.t = d_t; a.rh = d_rh;
  a.frq = dev_frq; a.airmass = dev_am;
  a.tb = d_tb; a.valid = d_valid;
  if (ex) { a.tbatm = ex->tbatm; a.tmr = ex->tmr; a.tauwet = ex->tauwet; a.taudry = ex->taudry; a.taulay = ex->taulay; }
  a.nlev = nlev; a.nf = nf; a.nang = nang;
  if (ex) { a.tauliq = ex->tauliq; a.tauice = ex->tauice; }
  // (clear sky: the kernel writes the cloud columns itself -- 0 x air mass for good rows, NaN for blanked profiles
  // and NaN elevations, like every other column)
  if (cloudy) { a.denliq = opt->denliq; a.denice = opt->denice; }
  if (ozone) a.o3n = opt->o3n;
  bool ws_held = false;                               // a shared workspace is in use: handed over on every return path
  auto handover = on_scope_exit([&] { if (ws_held) (void)workspace_release(c, st); });
  if (rays) {
    // RTEquation.refractivity + ray_tracing [EXT] as a pre-kernel on the same stream: path factor ds/dz per
    // (profile, angle, layer) into the context's workspace (grown only, never shrunk)
    const double* dev_elev = nullptr;
    rc = upload_small(c, c->elev_cache, elev, nang, &dev_elev); if (rc) return rc;
    HIP_TRY(grow_behind_drain(c->d_amf, (size_t)nprof * nang * nlev * sizeof(double)));
    HIP_TRY(grow_behind_drain(c->d_duct, (size_t)nprof));
    rc = workspace_acquire(c, st); if (rc) return rc;
    ws_held = true;
    HIP_TRY(hipMemsetAsync(c->d_duct.p, 0, (size_t)nprof, st));
    HIP_TRY(launch_ray_paths(d_z, d_p, d_t, d_rh, nprof, (int)nlev, dev_elev, (int)nang, c->d_amf.as<double>(),
                             c->d_duct.as<uint8_t>(), st));
    a.amf = c->d_amf.as<double>();
    a.duct = c->d_duct.as<uint8_t>();
  }
  bool extras = false;
  for (const ExtraSlot& x : EXTRA_SLOTS) extras = extras || (ex && ex->*x.col);
  int variant = extras ? FUSED_FULL : (use_opt ? FUSED_OPT : FUSED_TB_ONLY);
  if (from_alpha) {
    if (extras || use_opt || nmodels != 1)
      return fail(MWRT_ERR_UNSUPPORTED, "RTE from absorption: one model, no extras, no options");
    a.awet_in = d_awet; a.adry_in = d_adry;
    variant = FUSED_FROM_ALPHA;
  }
  // Fine spectral grids (BASELINE configs[4]): K1 -> tau -> K2.  The windowed absorption kernel (k_absorb_win) is
  // ~1.8x the fused kernel's K1 on such grids and ends each chunk with the layer step, so what crosses HBM is the
  // zenith layer optical depth: 8 B per (profile, level, frequency), written once, read once by k_rte_tau
  // (lane = frequency).  Profile batches of <= alpha_batch_bytes, both kernels on the caller's stream.
  if (variant == FUSED_TB_ONLY && nmodels == 1 &&
      absorption_route(c->absorption_mode, c->lds_max, frq, nf, tau_threads(nlev)) == AbsorbRoute::windowed) {
    const int fpitch = tau_pitch_of(nf);
    const size_t per_prof = (size_t)nlev * fpitch * sizeof(double);
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(nprof, (int64_t)(c->alpha_batch_bytes / per_prof)));
    const hipError_t e = grow_behind_drain(c->d_alpha, (size_t)batch * per_prof);
    if (e == hipErrorOutOfMemory) (void)hipGetLastError();          // no room for tau: the fused kernel needs no workspace at all
    else {
      HIP_TRY(e);
      rc = workspace_acquire(c, st); if (rc) return rc;
      ws_held = true;
      for (int64_t b0 = 0; b0 < nprof; b0 += batch) {
        const int64_t nb = std::min(batch, nprof - b0);
        double* d_tau = c->d_alpha.as<double>();
        rc = layer_tau_launch(c, ms[0], nb, nlev, d_z + b0 * nlev, d_p + b0 * nlev, d_t + b0 * nlev, d_rh + b0 * nlev, nf, frq,
                              dev_frq, d_tau, fpitch, d_valid + b0, st);
        if (rc) return rc;
        rc = rte_tau_launch(c, ms[0], nb, nlev, d_tau, fpitch, d_t + b0 * nlev, nf, dev_frq, nang, dev_am,
                            d_tb + (size_t)b0 * nang * nf, d_valid + b0, st);
        if (rc) return rc;
      }
      return MWRT_OK;
    }
  }
  const int nfc_main = pick_nfc_fused(c->chunk_width, c->lds_max, nlev, nf, nang);
  if (variant != FUSED_FROM_ALPHA)
    for (int i = 0; i < nmodels; ++i) { rc = get_masks(c, ms[i], frq, nf, nfc_main, &a.masks[i]); if (rc) return rc; }
  return launch_fused(c, nfc_main, a, rows, st, variant);
}

int mwrt_tb_batch_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                         const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                         int32_t nf, const double* frq, int32_t nang, const double* elev,
                         double* d_tb, uint8_t* d_valid, const mwrt_tb_extras* ex, void* stream) {
  if (!c || !m) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or model");
  return tb_launch(c, 1, &m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_valid, ex, stream);
}

int mwrt_tb_batch_opt_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                             const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                             int32_t nf, const double* frq, int32_t nang, const double* elev,
                             double* d_tb, uint8_t* d_valid, const mwrt_tb_extras* ex, const mwrt_tb_options* opt,
                             void* stream) {
  if (!c || !m) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or model");
  return tb_launch(c, 1, &m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_valid, ex, stream, opt);
}

int mwrt_tb_from_absorption_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                   const double* d_z, const double* d_t, int32_t nf, const double* frq, int32_t nang,
                                   const double* elev, const double* d_awet, const double* d_adry,
                                   double* d_tb, uint8_t* d_valid, void* stream) {
  if (!c || !m) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or model");
  if (!d_awet || !d_adry) return fail(MWRT_ERR_INVALID_ARGUMENT, "null buffer");
  return tb_launch(c, 1, &m, nprof, nlev, d_z, nullptr, d_t, nullptr, nf, frq, nang, elev, d_tb, d_valid, nullptr, stream,
                   nullptr, d_awet, d_adry);
}

int mwrt_tb_batch_multi_device(mwrt_context* c, int32_t nmodels, const mwrt_model* const* models, int64_t nprof,
                               int32_t nlev, const double* d_z, const double* d_p, const double* d_t,
                               const double* d_rh, int32_t nf, const double* frq, int32_t nang, const double* elev,
                               double* d_tb, uint8_t* d_valid, void* stream) {
  if (!c) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context");
  return tb_launch(c, nmodels, models, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_valid, nullptr,
                   stream);
}

// the host-buffer TB entries behind their checks: the profiles cross PCIe once (for all models), one tb_launch, the
// results come back and flagged rows are blanked
static int tb_host(mwrt_context* c, hipStream_t st, int nmodels, const mwrt_model* const* ms, int64_t nprof, int32_t nlev,
                   const double* z, const double* p, const double* t, const double* rh, int32_t nf, const double* frq,
                   int32_t nang, const double* elev, double* tb, uint8_t* valid, const mwrt_tb_extras* ex,
                   const mwrt_tb_options* opt) {
  const size_t nin = (size_t)nprof * nlev, rows = (size_t)nprof * nmodels, nout = rows * nang * nf;
  // inputs: z p t rh, then whichever of denliq denice o3n the options carry
  const double* src[7] = {z, p, t, rh};
  int nsrc = 4;
  mwrt_tb_options dopt{};
  const double** dopt_in[3] = {&dopt.denliq, &dopt.denice, &dopt.o3n};
  const double* opt_in[3] = {opt ? opt->denliq : nullptr, opt ? opt->denice : nullptr, opt ? opt->o3n : nullptr};
  int where[3];
  for (int k = 0; k < 3; ++k) if (opt_in[k]) { where[k] = nsrc; src[nsrc++] = opt_in[k]; }
  int rc = stage_in(c, st, nin, src, nsrc); if (rc) return rc;
  HIP_TRY(c->d_out.reserve(nout * sizeof(double)));
  HIP_TRY(c->d_valid.reserve(rows));
  const double* din = c->d_in.as<double>();
  for (int k = 0; k < 3; ++k) if (opt_in[k]) *dopt_in[k] = din + (size_t)where[k] * nin;
  if (opt) dopt.ray_tracing = opt->ray_tracing;
  mwrt_tb_extras dex{};
  if (ex) {
    size_t need = 0;
    for (const ExtraSlot& x : EXTRA_SLOTS) if (ex->*x.col) need += rows * x.row(nlev, nf, nang);
    HIP_TRY(c->d_ex.reserve(need * sizeof(double) + 8));
    double* q = c->d_ex.as<double>();
    for (const ExtraSlot& x : EXTRA_SLOTS) if (ex->*x.col) { dex.*x.col = q; q += rows * x.row(nlev, nf, nang); }
  }
  rc = tb_launch(c, nmodels, ms, nprof, nlev, din, din + nin, din + 2 * nin, din + 3 * nin, nf, frq, nang, elev,
                 c->d_out.as<double>(), c->d_valid.as<uint8_t>(), ex ? &dex : nullptr, st, opt ? &dopt : nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(tb, c->d_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(valid, c->d_valid.p, rows, hipMemcpyDeviceToHost, st));
  // a profile flagged 2 (negative absorption: pyrtlib raises for the whole execute()) is blanked
  // as a whole, whichever frequency chunk met it
  RowArray out[1 + NEX] = {{tb, (size_t)nang * nf}};
  int nout_arrays = 1;
  for (const ExtraSlot& x : EXTRA_SLOTS) {
    if (!ex || !(ex->*x.col)) continue;
    const size_t per = x.row(nlev, nf, nang);
    HIP_TRY(hipMemcpyAsync(ex->*x.col, dex.*x.col, rows * per * sizeof(double), hipMemcpyDeviceToHost, st));
    out[nout_arrays++] = RowArray{ex->*x.col, per};
  }
  HIP_TRY(hipStreamSynchronize(st));
  blank_rows(valid, (int64_t)rows, out, nout_arrays);
  return MWRT_OK;
}

int mwrt_tb_batch_multi(mwrt_context* c, int32_t nmodels, const mwrt_model* const* models, int64_t nprof, int32_t nlev,
                        const double* z, const double* p, const double* t, const double* rh,
                        int32_t nf, const double* frq, int32_t nang, const double* elev,
                        double* tb, uint8_t* valid) {
  if (!c || !models || nmodels < 1 || nmodels > MAX_MULTI) return fail(MWRT_ERR_INVALID_ARGUMENT, "bad context / models");
  if (!z || !p || !t || !rh || !frq || !elev || !tb || !valid) return fail(MWRT_ERR_INVALID_ARGUMENT, "null buffer");
  if (nprof < 0 || nlev < 2 || nf < 1 || nang < 1) return fail(MWRT_ERR_INVALID_ARGUMENT, "bad sizes");
  if (nprof == 0) return MWRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  return tb_host(c, c->stream, nmodels, models, nprof, nlev, z, p, t, rh, nf, frq, nang, elev, tb, valid, nullptr, nullptr);
}

int mwrt_tb_batch(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                  const double* z, const double* p, const double* t, const double* rh,
                  int32_t nf, const double* frq, int32_t nang, const double* elev,
                  double* tb, uint8_t* valid, const mwrt_tb_extras* ex) {
  return mwrt_tb_batch_opt(c, m, nprof, nlev, z, p, t, rh, nf, frq, nang, elev, tb, valid, ex, nullptr);
}

int mwrt_tb_batch_opt(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                      const double* z, const double* p, const double* t, const double* rh,
                      int32_t nf, const double* frq, int32_t nang, const double* elev,
                      double* tb, uint8_t* valid, const mwrt_tb_extras* ex, const mwrt_tb_options* opt) {
  CallSpec s{CALL_ANGLES | CALL_HOST | CALL_STAGES, nprof, nlev, nf, frq, nang, elev, nullptr};
  s.buffers_ok = z && p && t && rh && frq && elev && tb && valid;
  Call call;
  const int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  return tb_host(c, call.st, 1, &m, nprof, nlev, z, p, t, rh, nf, frq, nang, elev, tb, valid, ex, opt);
}

int mwrt_absorption_batch_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                 const double* d_p, const double* d_t, const double* d_rh,
                                 int32_t nf, const double* frq, double* d_awet, double* d_adry, void* stream) {
  CallSpec s{0, nprof, nlev, nf, frq, 0, nullptr, stream};
  s.buffers_ok = d_p && d_t && d_rh && frq && d_awet && d_adry;
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  const int wthreads = lanes_for(nlev);                 // node sums in LDS: 2 x 16 doubles per thread
  const AbsorbRoute route = absorption_route(c->absorption_mode, c->lds_max, frq, nf, wthreads);
  if (route == AbsorbRoute::refused)
    return fail(MWRT_ERR_UNSUPPORTED, "windowed absorption needs >= 128 strictly increasing frequencies in windows <= 6 GHz wide");
  if (route == AbsorbRoute::windowed)
    return launch_windowed_absorption(c, m, nprof, nlev, d_p, d_t, d_rh, nf, frq, call.dev_frq, d_awet, d_adry, nullptr, wthreads,
                                      call.st);
  AbsorbArgs a{};
  a.M = m->d_desc; a.p = d_p; a.t = d_t; a.rh = d_rh; a.frq = call.dev_frq;
  a.awet = d_awet; a.adry = d_adry; a.nlev = nlev; a.nf = nf;
  rc = get_masks(c, m, frq, nf, pick_nfc(nf), &a.masks); if (rc) return rc;
  return launch_absorb(c, pick_nfc(nf), a, nprof, call.st);
}

int mwrt_absorption_batch(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                          const double* p, const double* t, const double* rh,
                          int32_t nf, const double* frq, double* awet, double* adry) {
  CallSpec s{CALL_HOST | CALL_STAGES, nprof, nlev, nf, frq, 0, nullptr, nullptr};
  s.buffers_ok = p && t && rh && frq && awet && adry;
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  hipStream_t st = call.st;
  const size_t nin = (size_t)nprof * nlev, nout = (size_t)nprof * nf * nlev;
  const double* src[3] = {p, t, rh};
  rc = stage_in(c, st, nin, src, 3); if (rc) return rc;
  HIP_TRY(c->d_out.reserve(2 * nout * sizeof(double)));
  const double* din = c->d_in.as<double>();
  double* dout = c->d_out.as<double>();
  rc = mwrt_absorption_batch_device(c, m, nprof, nlev, din, din + nin, din + 2 * nin, nf, frq, dout, dout + nout, st);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(awet, dout, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(adry, dout + nout, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MWRT_OK;
}

int mwrt_layer_tau_pitch(int32_t nf) { return nf < 1 ? 0 : tau_pitch_of(nf); }

int mwrt_layer_tau_batch_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                                int32_t nf, const double* frq, double* d_tau, int32_t tau_pitch, uint8_t* d_valid,
                                void* stream) {
  CallSpec s{0, nprof, nlev, nf, frq, 0, nullptr, stream};
  s.buffers_ok = d_z && d_p && d_t && d_rh && frq && d_tau && d_valid;
  if (tau_pitch < tau_pitch_of(nf) || tau_pitch % TAU_NFC != 0)
    s.after_buffers = Check{MWRT_ERR_INVALID_ARGUMENT, "tau_pitch must be a multiple of 16 and >= mwrt_layer_tau_pitch(nf)"};
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  return layer_tau_launch(c, m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, call.dev_frq, d_tau, tau_pitch, d_valid, call.st);
}

int mwrt_tb_from_layer_tau_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                  const double* d_tau, int32_t tau_pitch, const double* d_t,
                                  int32_t nf, const double* frq, int32_t nang, const double* elev,
                                  const uint8_t* d_valid, double* d_tb, void* stream) {
  CallSpec s{CALL_ANGLES, nprof, nlev, nf, frq, nang, elev, stream};
  s.buffers_ok = d_tau && d_t && frq && elev && d_valid && d_tb;
  if (tau_pitch < nf) s.after_buffers = Check{MWRT_ERR_INVALID_ARGUMENT, "tau_pitch < nf"};
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  return rte_tau_launch(c, m, nprof, nlev, d_tau, tau_pitch, d_t, nf, call.dev_frq, nang, call.dev_am, d_tb, d_valid, call.st);
}

// Tangent-linear absorption (k_absorb_tl): alpha and d alpha / dT|e, d alpha / de|T.  DEVICE buffers, asynchronous.
int mwrt_absorption_tl_batch_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                    const double* d_p, const double* d_t, const double* d_rh, int32_t nf, const double* frq,
                                    double* d_awet, double* d_adry, double* d_dawet_dt, double* d_dawet_de,
                                    double* d_dadry_dt, double* d_dadry_de, void* stream) {
  CallSpec s{0, nprof, nlev, nf, frq, 0, nullptr, stream};
  s.buffers_ok = d_p && d_t && d_rh && frq && d_awet && d_adry && d_dawet_dt && d_dawet_de && d_dadry_dt && d_dadry_de;
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  AbsorbTlArgs a{};
  a.M = m->d_desc; a.p = d_p; a.t = d_t; a.rh = d_rh; a.frq = call.dev_frq;
  a.awet = d_awet; a.adry = d_adry; a.dawet_dt = d_dawet_dt; a.dawet_de = d_dawet_de; a.dadry_dt = d_dadry_dt; a.dadry_de = d_dadry_de;
  a.flags = nullptr; a.nlev = nlev; a.nf = nf; a.nslab = (nlev + WAVE - 1) / WAVE;
  return timed(c, call.st, [&] { return launch_absorb_tl(a, nprof, call.st); });
}

// The K-matrix on caller-owned HBM: k_absorb_tl into the context's workspace, then k_jac_rte.  Asynchronous; after one
// warm-up call with the same shapes and frequencies it neither allocates nor synchronises.
int mwrt_tb_jacobian_batch_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                  const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                                  int32_t nf, const double* frq, int32_t nang, const double* elev,
                                  double* d_tb, double* d_dtb_dt, double* d_dtb_de, double* d_dtb_ddz, uint8_t* d_valid,
                                  void* stream) {
  return mwrt_tb_jacobian_batch_opt_device(c, m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_dtb_dt,
                                           d_dtb_de, d_dtb_ddz, nullptr, nullptr, d_valid, nullptr, stream);
}

// The same with cloud liquid / ice (mwrt_tb_options.denliq / denice, device pointers): k_jac_rte forms the cloud
// absorption and its tangents itself, so the workspace and the launches are those of the clear call.
int mwrt_tb_jacobian_batch_opt_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                      const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                                      int32_t nf, const double* frq, int32_t nang, const double* elev,
                                      double* d_tb, double* d_dtb_dt, double* d_dtb_de, double* d_dtb_ddz,
                                      double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                                      const mwrt_tb_options* opt, void* stream) {
  // (this entry has no optional thickness row: the check sits where its "null buffer" check always sat)
  return jacobian_vars_device(c, m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_dtb_dt, d_dtb_de, d_dtb_ddz,
                              d_dtb_dliq, d_dtb_dice, d_valid, opt, nullptr, /*ddz_required=*/true, /*ray=*/false, stream);
}

// The same in the caller's retrieval variables (mwrt_jac_variables): k_jac_rte changes the variables of each row element
// before it stores it, so there is no further launch, no further workspace and no second pass over the rows.
int mwrt_tb_jacobian_batch_vars_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                       const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                                       int32_t nf, const double* frq, int32_t nang, const double* elev,
                                       double* d_tb, double* d_dtb_dt, double* d_dtb_dh, double* d_dtb_ddz,
                                       double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                                       const mwrt_tb_options* opt, const mwrt_jac_variables* vars, void* stream) {
  return jacobian_vars_device(c, m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_dtb_dt, d_dtb_dh, d_dtb_ddz,
                              d_dtb_dliq, d_dtb_dice, d_valid, opt, vars, /*ddz_required=*/false, /*ray=*/false, stream);
}

// ... and on HOST buffers, synchronous (jacobian_vars_host).
int mwrt_tb_jacobian_batch_vars(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                const double* z, const double* p, const double* t, const double* rh,
                                int32_t nf, const double* frq, int32_t nang, const double* elev,
                                double* tb, double* dtb_dt, double* dtb_dh, double* dtb_ddz, double* dtb_dliq, double* dtb_dice,
                                uint8_t* valid, const mwrt_tb_options* opt, const mwrt_jac_variables* vars) {
  return jacobian_vars_host(c, m, nprof, nlev, z, p, t, rh, nf, frq, nang, elev, tb, dtb_dt, dtb_dh, dtb_ddz, dtb_dliq, dtb_dice,
                            valid, opt, vars, /*ddz_required=*/false, /*ray=*/false);
}

// The K-matrix along refracted spherical ray paths: the operator of mwrt_tb_batch_opt_device with
// ray_tracing = 1 and its exact rows, the response of every layer's path factor to the refractive index and the heights
// included.  ray::k_ray_paths_tl into the context's path workspace, k_absorb_tl, then ray::k_jac_rte_ray; asynchronous, and
// after one warm-up call with the same shapes it neither allocates nor synchronises.
int mwrt_tb_jacobian_batch_ray_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                      const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                                      int32_t nf, const double* frq, int32_t nang, const double* elev,
                                      double* d_tb, double* d_dtb_dt, double* d_dtb_dh, double* d_dtb_ddz,
                                      double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                                      const mwrt_tb_options* opt, const mwrt_jac_variables* vars, void* stream) {
  return jacobian_vars_device(c, m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, d_tb, d_dtb_dt, d_dtb_dh, d_dtb_ddz,
                              d_dtb_dliq, d_dtb_dice, d_valid, opt, vars, /*ddz_required=*/false, /*ray=*/true, stream);
}

// ... and on HOST buffers, synchronous (jacobian_vars_host).
int mwrt_tb_jacobian_batch_ray(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                               const double* z, const double* p, const double* t, const double* rh,
                               int32_t nf, const double* frq, int32_t nang, const double* elev,
                               double* tb, double* dtb_dt, double* dtb_dh, double* dtb_ddz, double* dtb_dliq, double* dtb_dice,
                               uint8_t* valid, const mwrt_tb_options* opt, const mwrt_jac_variables* vars) {
  return jacobian_vars_host(c, m, nprof, nlev, z, p, t, rh, nf, frq, nang, elev, tb, dtb_dt, dtb_dh, dtb_ddz, dtb_dliq, dtb_dice,
                            valid, opt, vars, /*ddz_required=*/false, /*ray=*/true);
}

// The clear-sky K-matrix in the operator's own variables (T at fixed e, e, layer thickness) on HOST buffers: the call
// above without cloud, options or variables, and with all three rows required.
int mwrt_tb_jacobian_batch(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                           const double* z, const double* p, const double* t, const double* rh,
                           int32_t nf, const double* frq, int32_t nang, const double* elev,
                           double* tb, double* dtb_dt, double* dtb_de, double* dtb_ddz, uint8_t* valid) {
  return jacobian_vars_host(c, m, nprof, nlev, z, p, t, rh, nf, frq, nang, elev, tb, dtb_dt, dtb_de, dtb_ddz, nullptr, nullptr,
                            valid, nullptr, nullptr, /*ddz_required=*/true, /*ray=*/false);
}

// ---- the spectroscopic-parameter Jacobian (csrc/mwrt_par.hip) ----
namespace {

bool param_is_o2(int field) { return field == MWRT_PAR_O2_X || field == MWRT_PAR_O2_WB300 || field >= MWRT_PAR_O2_S300; }

// what is wrong with a parameter list for this model, or null
const char* check_params(const mwrt_model* m, int32_t npar, const mwrt_param* params) {
  if (npar < 1 || npar > MWRT_MAX_PARAMS) return "npar outside 1 .. MWRT_MAX_PARAMS";
  if (!params) return "null buffer";
  for (int i = 0; i < npar; ++i) {
    const int f = params[i].field, l = params[i].line;
    if (f < 0 || f >= MWRT_PAR_NFIELDS) return "unknown parameter field";
    if (f < MWRT_PAR_H2O_S1) {
      if (l != 0) return "line != 0 on a scalar parameter field";
      continue;
    }
    const int n = f < MWRT_PAR_O2_S300 ? m->h_desc.n_h2o : m->h_desc.n_o2;
    if (l != MWRT_PAR_ALL_LINES && (l < 0 || l >= n)) return "parameter line outside the model's table";
  }
  return nullptr;
}

// k_absorb_tl into the K-matrix workspace, then per group of parameters k_par_tangent and k_par_contract
int param_jacobian_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                          const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                          int32_t nf, const double* frq, int32_t nang, const double* elev,
                          int32_t npar, const mwrt_param* params, double* d_tb, double* d_dtb_db, uint8_t* d_valid,
                          void* stream) {
  if (!c || !m) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context or model");
  CallSpec s{CALL_ANGLES, nprof, nlev, nf, frq, nang, elev, stream};
  if (const char* bad = check_params(m, npar, params)) s.after_common = Check{MWRT_ERR_INVALID_ARGUMENT, bad};
  s.buffers_ok = d_z && d_p && d_t && d_rh && frq && elev && d_dtb_db && d_valid;
  const int nslab = (nlev + WAVE - 1) / WAVE;
  if (nprof * nf * nslab > 2147483647LL) s.before_device = Check{MWRT_ERR_UNSUPPORTED, "nprof x nf x level slabs exceeds grid limit"};
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  hipStream_t st = call.st;
  // the parameter list, content-keyed like the frequencies (field and line as one exactly representable double each)
  std::vector<double> key((size_t)npar);
  for (int i = 0; i < npar; ++i) key[(size_t)i] = params[i].field * 1024.0 + (params[i].line + 1);
  DeviceCache::Blob pb;
  HIP_TRY(c->par_cache.get(0, 0, key.data(), npar, c->stream, [&](std::vector<char>* host) {
    host->assign((const char*)params, (const char*)(params + npar));
    return npar;
  }, &pb));
  const mwrt_param* dev_par = (const mwrt_param*)pb.dev;
  const size_t nabs = (size_t)nprof * nf * nlev;
  size_t gmax = par::PAR_WS_BYTES / (sizeof(double) * nabs);
  gmax = gmax < 1 ? 1 : (gmax > (size_t)npar ? (size_t)npar : gmax);
  HIP_TRY(grow_behind_drain(c->d_jac, sizeof(double) * 6 * nabs + sizeof(unsigned) * (size_t)nprof));
  HIP_TRY(grow_behind_drain(c->d_par, sizeof(double) * nabs * gmax));
  rc = workspace_acquire(c, st); if (rc) return rc;
  auto handover = on_scope_exit([&] { (void)workspace_release(c, st); });    // on every return path from here on
  double* w = c->d_jac.as<double>();
  unsigned* flags = reinterpret_cast<unsigned*>(w + 6 * nabs);
  HIP_TRY(hipMemsetAsync(flags, 0, sizeof(unsigned) * (size_t)nprof, st));
  AbsorbTlArgs ta{};
  ta.M = m->d_desc; ta.p = d_p; ta.t = d_t; ta.rh = d_rh; ta.frq = call.dev_frq;
  ta.awet = w; ta.adry = w + nabs; ta.dawet_dt = w + 2 * nabs; ta.dawet_de = w + 3 * nabs;
  ta.dadry_dt = w + 4 * nabs; ta.dadry_de = w + 5 * nabs;
  ta.flags = flags; ta.nlev = nlev; ta.nf = nf; ta.nslab = nslab;
  rc = timed(c, st, [&] { return launch_absorb_tl(ta, nprof, st); });
  if (rc) return rc;
  for (int p0 = 0; p0 < npar; p0 += (int)gmax) {
    const int gn = npar - p0 < (int)gmax ? npar - p0 : (int)gmax;
    par::ParTangentArgs pt{};
    pt.M = m->d_desc; pt.p = d_p; pt.t = d_t; pt.rh = d_rh; pt.frq = call.dev_frq; pt.params = dev_par;
    pt.dalpha = c->d_par.as<double>(); pt.nlev = nlev; pt.nf = nf; pt.nslab = nslab; pt.p0 = p0; pt.gn = gn;
    for (int q = p0; q < p0 + gn; ++q) pt.o2_any |= param_is_o2(params[q].field) ? 1 : 0;
    rc = timed(c, st, [&] { return par::launch_par_tangent(pt, nprof, st); });
    if (rc) return rc;
    par::ParContractArgs pc{};
    pc.M = m->d_desc; pc.z = d_z; pc.t = d_t; pc.awet = ta.awet; pc.adry = ta.adry; pc.flags = flags;
    pc.frq = call.dev_frq; pc.airmass = call.dev_am; pc.params = dev_par; pc.dalpha = pt.dalpha;
    pc.tb = d_tb; pc.dtb_db = d_dtb_db; pc.valid = d_valid;
    pc.nlev = nlev; pc.nf = nf; pc.nang = nang; pc.npar = npar; pc.p0 = p0; pc.gn = gn;
    rc = timed(c, st, [&] { return par::launch_par_contract(pc, nprof, st); });
    if (rc) return rc;
  }
  return MWRT_OK;
}

}  // namespace

int mwrt_tb_param_jacobian_batch_device(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                        const double* d_z, const double* d_p, const double* d_t, const double* d_rh,
                                        int32_t nf, const double* frq, int32_t nang, const double* elev,
                                        int32_t npar, const mwrt_param* params,
                                        double* d_tb, double* d_dtb_db, uint8_t* d_valid, void* stream) {
  return param_jacobian_device(c, m, nprof, nlev, d_z, d_p, d_t, d_rh, nf, frq, nang, elev, npar, params, d_tb, d_dtb_db,
                               d_valid, stream);
}

// ... and on HOST buffers, synchronous: staged through a device buffer of this call's own (freed on every return path), one
// param_jacobian_device call on the context's stream -- which makes every check and every decision -- and the results
// copied back as they are.
int mwrt_tb_param_jacobian_batch(mwrt_context* c, const mwrt_model* m, int64_t nprof, int32_t nlev,
                                 const double* z, const double* p, const double* t, const double* rh,
                                 int32_t nf, const double* frq, int32_t nang, const double* elev,
                                 int32_t npar, const mwrt_param* params, double* tb, double* dtb_db, uint8_t* valid) {
  CallSpec s{CALL_ANGLES | CALL_HOST | CALL_STAGES, nprof, nlev, nf, frq, nang, elev, nullptr};
  if (npar < 1 || npar > MWRT_MAX_PARAMS) s.after_common = Check{MWRT_ERR_INVALID_ARGUMENT, "npar outside 1 .. MWRT_MAX_PARAMS"};
  s.buffers_ok = z && p && t && rh && frq && elev && params && dtb_db && valid;
  Call call;
  int rc = begin_call(c, &m, 1, s, &call);
  if (rc || call.empty) return rc;
  hipStream_t st = call.st;
  const size_t nin = (size_t)nprof * nlev, ntb = (size_t)nprof * nang * nf, nout = ntb * (size_t)npar;
  DevBuf buf;                                                     // this call's own: inputs | tb | columns | valid
  auto free_buf = on_scope_exit([&] { buf.release(); });
  HIP_TRY(buf.reserve(sizeof(double) * (4 * nin + ntb + nout) + (size_t)nprof));
  double* q = buf.as<double>();
  const double* in[4] = {z, p, t, rh};
  const double* din[4] = {};
  for (int k = 0; k < 4; ++k) {
    HIP_TRY(hipMemcpyAsync(q, in[k], sizeof(double) * nin, hipMemcpyHostToDevice, st));
    din[k] = q; q += nin;
  }
  double* d_tb = q; q += ntb;
  double* d_out = q; q += nout;
  uint8_t* d_valid = reinterpret_cast<uint8_t*>(q);
  rc = param_jacobian_device(c, m, nprof, nlev, din[0], din[1], din[2], din[3], nf, frq, nang, elev, npar, params,
                             d_tb, d_out, d_valid, nullptr);
  if (rc) return rc;
  if (tb) HIP_TRY(hipMemcpyAsync(tb, d_tb, sizeof(double) * ntb, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(dtb_db, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(valid, d_valid, (size_t)nprof, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MWRT_OK;
}

int mwrt_set_chunk_width(mwrt_context* c, int width) {
  if (!c) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context");
  if (width != 0 && width != 8 && width != 14 && width != 16) return fail(MWRT_ERR_INVALID_ARGUMENT, "chunk width: 0 (automatic), 8, 14 or 16");
  c->chunk_width = width;
  return MWRT_OK;
}

int mwrt_set_absorption_mode(mwrt_context* c, int mode) {
  if (!c || mode < 0 || mode > 2) return fail(MWRT_ERR_INVALID_ARGUMENT, "mode must be 0, 1 or 2");
  c->absorption_mode = mode;
  return MWRT_OK;
}

int mwrt_selftest_math(mwrt_context* c, int32_t n, const double* x, const double* y_pos,
                       double* exp_x, double* log_y, double* x_div_y, double* x_div1_y) {
  if (!c || n < 0 || !x || !y_pos || !exp_x || !log_y || !x_div_y || !x_div1_y)
    return fail(MWRT_ERR_INVALID_ARGUMENT, "null argument");
  if (n == 0) return MWRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t b = sizeof(double) * (size_t)n;
  const double* src[2] = {x, y_pos};
  int rc = stage_in(c, c->stream, (size_t)n, src, 2); if (rc) return rc;
  HIP_TRY(c->d_out.reserve(4 * b));
  double* din = c->d_in.as<double>();
  double* dout = c->d_out.as<double>();
  HIP_TRY(launch_selftest_math(din, din + n, dout, dout + n, dout + 2 * (size_t)n, dout + 3 * (size_t)n, n, c->stream));
  double* dst[4] = {exp_x, log_y, x_div_y, x_div1_y};
  for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(dst[k], dout + (size_t)k * n, b, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MWRT_OK;
}

int mwrt_selftest_helpers(mwrt_context* c, int32_t helper, int32_t n, int32_t block,
                          const double* in0, const double* in1, const double* in2, const double* in3,
                          double* out0, double* out1, double* out2, double* out3, uint8_t* flag) {
  if (!c) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context");
  if (helper < 0 || helper >= MWRT_HELPER_COUNT) return fail(MWRT_ERR_INVALID_ARGUMENT, "selftest_helpers: unknown helper");
  if (n < 0) return fail(MWRT_ERR_INVALID_ARGUMENT, "selftest_helpers: n < 0");
  if (block < 64 || block > 1024 || block % 64 != 0)
    return fail(MWRT_ERR_INVALID_ARGUMENT, "selftest_helpers: block must be a multiple of 64 in 64..1024");
  if (helper == MWRT_HELPER_LAYER_VALUE4 && n % 4 != 0)
    return fail(MWRT_ERR_INVALID_ARGUMENT, "selftest_helpers: LAYER_VALUE4 takes n in multiples of 4");
  if (n == 0) return MWRT_OK;
  if (!flag) return fail(MWRT_ERR_INVALID_ARGUMENT, "selftest_helpers: null flag");
  HIP_TRY(hipSetDevice(c->device));
  const size_t b = sizeof(double) * (size_t)n;
  const std::vector<double> zeros((size_t)n, 0.0);
  std::vector<double> magic;
  if (helper == MWRT_HELPER_DIV_SMALL) {                // the magic number as the planning code makes it
    if (!in1) return fail(MWRT_ERR_INVALID_ARGUMENT, "selftest_helpers: DIV_SMALL needs in1 (the divisors)");
    magic.resize((size_t)n);
    for (int32_t i = 0; i < n; ++i) magic[i] = (double)magic_of((int)in1[i]);
    in2 = magic.data();
  }
  const double* src[4] = {in0 ? in0 : zeros.data(), in1 ? in1 : zeros.data(), in2 ? in2 : zeros.data(),
                          in3 ? in3 : zeros.data()};
  int rc = stage_in(c, c->stream, (size_t)n, src, 4); if (rc) return rc;
  HIP_TRY(c->d_out.reserve(4 * b + (size_t)n));
  double* din = c->d_in.as<double>();
  double* dout = c->d_out.as<double>();
  HIP_TRY(hipMemsetAsync(dout, 0, 4 * b + (size_t)n, c->stream));
  HelperArgs a;
  for (int k = 0; k < 4; ++k) { a.in[k] = din + (size_t)k * n; a.out[k] = dout + (size_t)k * n; }
  a.flag = reinterpret_cast<uint8_t*>(dout + 4 * (size_t)n);
  a.n = n; a.helper = helper;
  HIP_TRY(launch_selftest_helpers(a, block, c->stream));
  double* dst[4] = {out0, out1, out2, out3};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], a.out[k], b, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(flag, a.flag, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));                // (the staged host vectors live until here)
  return MWRT_OK;
}

int mwrt_synchronize(mwrt_context* c, void* stream) {
  if (!c) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(resolve_stream(c, stream)));
  return MWRT_OK;
}

int mwrt_set_timing(mwrt_context* c, int enabled) {
  if (!c) return fail(MWRT_ERR_INVALID_ARGUMENT, "null context");
  HIP_TRY(hipSetDevice(c->device));
  if (enabled && c->ev0.empty()) {
    c->ev0.resize(TIMING_RING); c->ev1.resize(TIMING_RING);
    for (int i = 0; i < TIMING_RING; ++i) { HIP_TRY(hipEventCreate(&c->ev0[i])); HIP_TRY(hipEventCreate(&c->ev1[i])); }
  }
  c->timing = enabled != 0;
  c->ev_count = 0;
  return MWRT_OK;
}

int mwrt_timing_collect(mwrt_context* c, double* total_ms, int32_t* launches) {
  if (!c || !total_ms || !launches) return fail(MWRT_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  const long n = c->ev_count < TIMING_RING ? c->ev_count : TIMING_RING;
  double sum = 0.0;
  for (long i = 0; i < n; ++i) {
    HIP_TRY(hipEventSynchronize(c->ev1[i]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]));
    sum += ms;
  }
  *total_ms = sum;
  *launches = (int32_t)n;
  c->ev_count = 0;
  return MWRT_OK;
}

int mwrt_last_kernel_ms(mwrt_context* c, double* ms_out) {
  if (!c || !ms_out) return fail(MWRT_ERR_INVALID_ARGUMENT, "null argument");
  if (c->ev_count < 1) return fail(MWRT_ERR_INVALID_ARGUMENT, "no timed launch pending");
  const long i = (c->ev_count - 1) % TIMING_RING;
  HIP_TRY(hipEventSynchronize(c->ev1[i]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]));
  *ms_out = ms;
  return MWRT_OK;
}

}  // extern "C"
