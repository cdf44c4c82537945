// mwrt_par.hip -- the spectroscopic-parameter Jacobian d TB / d b (include/mwrt.h mwrt_tb_param_jacobian_batch_device;
// declarations: mwrt_par.hip.h; the mathematics: DESIGN.md section 4.8).
//
//   d TB / d b = sum over levels l of  s_wet_l * d awet_l / d b  +  s_dry_l * d adry_l / d b
//
// s_wet_l, s_dry_l = d TB / d alpha_l are what k_jac_rte multiplies its absorption tangents with (level l as the upper end
// of layer l and as the lower end of layer l + 1); d alpha_l / d b is the tangent of k_absorb_tl's absorption with the seed
// on a table entry instead of on T or e.  Each parameter touches one species only.
#include "mwrt_par.hip.h"
#include "mwrt_absorption.hip.h"      // level_state, goff_gratch_e (and the arithmetic of mwrt_math.hip.h)
#include "mwrt_tl_dev.hip.h"          // hui_w_dw, layer_value_tl, the workgroup scans (shared with mwrt_tl.hip)

namespace mwrt {
namespace par {

namespace {

// ---------------------------------------------------------------------------------------------
// Forward-mode tangent in ONE direction: value, d / d b
// ---------------------------------------------------------------------------------------------
struct du { double v, d; };
__device__ __forceinline__ du operator+(du a, du b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ du operator-(du a, du b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ du operator*(du a, du b) { return {a.v * b.v, __builtin_fma(a.d, b.v, a.v * b.d)}; }
__device__ __forceinline__ du operator*(double s, du a) { return {s * a.v, s * a.d}; }
__device__ __forceinline__ du operator+(du a, double s) { return {a.v + s, a.d}; }
__device__ __forceinline__ du operator+(double s, du a) { return {a.v + s, a.d}; }
__device__ __forceinline__ du udiv(du a, du b) {
  const double r = fdiv(1.0, b.v), q = a.v * r;
  return {q, (a.d - q * b.d) * r};
}
__device__ __forceinline__ du uexp(du a) { const double v = fexp(a.v); return {v, v * a.d}; }

// a table entry and its seed: 1 per unit of the entry as mwrt_model_desc stores it (`unit`: the device image keeps S / F^2),
// or the entry itself under MWRT_PAR_ALL_LINES (a common factor s on every line: d (s b_k) / ds at s = 1)
__device__ __forceinline__ du entry(double val, bool hit, bool all, double unit = 1.0) {
  return {val, hit ? (all ? val : unit) : 0.0};
}

__device__ __forceinline__ bool is_wet(int field) { return field <= MWRT_PAR_H2O_XCS || (field >= MWRT_PAR_H2O_S1 && field <= MWRT_PAR_H2O_SHS); }

// what k_absorb_tl forms per level before its line loops (the values alone)
struct Level {
  double t, P, rho, pdry;
  double pvap, pda, tiln, ti, ti2, lnc;             // H2O
  double th, th1, lnth, b, presda, preswv;          // O2
};

__device__ __forceinline__ Level level_of(cmodel M, double pin, double tin, double rhin) {
  const LevelState L = level_state(pin, tin, goff_gratch_e(tin, rhin));
  Level S;
  S.t = L.t; S.P = L.p; S.rho = L.rho; S.pdry = L.pdry;
  S.pvap = fdiv(1.0, M->h2o_pvap_div) * (L.rho * L.t);
  S.pda = L.p - S.pvap;
  S.lnc = flog(fdiv(M->h2o_reftcon, L.t));
  S.ti = fdiv(M->h2o_reftline, L.t);
  S.tiln = flog(S.ti);
  S.ti2 = fexp(2.5 * S.tiln);
  S.th = fdiv(300.0, L.t);
  S.th1 = S.th - 1.0;
  S.lnth = flog(S.th);
  S.b = fexp(M->o2_x * S.lnth);
  S.preswv = fdiv(1.0, M->o2_pvap_div) * (L.rho * L.t);
  S.presda = L.p - S.preswv;
  return S;
}

// H2O line k's term of k_absorb_tl's `sum` (before f^2 * 3.183e-05 den), with the seed of `field` on this line.  The
// branches (750-GHz cutoffs, the speed-dependent switch) are taken on the values, as the forward takes them.
__device__ __forceinline__ du h2o_line(cmodel M, int k, int field, bool all, const Level& S, double f) {
  const auto& R = M->h2or[k];
  const du rw0 = entry(R.w0, field == MWRT_PAR_H2O_W0, all), rx = entry(R.x, field == MWRT_PAR_H2O_X, all);
  const du rw0s = entry(R.w0s, field == MWRT_PAR_H2O_W0S, all), rxs = entry(R.xs, field == MWRT_PAR_H2O_XS, all);
  const du w0 = rw0 * (S.pda * uexp(S.tiln * rx)) + rw0s * (S.pvap * uexp(S.tiln * rxs));
  du c1 = {R.fl, 0.0};
  if (M->h2o_shift_mode != 0) {
    double af = S.pda, as = S.pvap;
    if (R.aair != 0.0) af *= 1.0 - R.aair * S.tiln;
    if (R.aself != 0.0) as *= 1.0 - R.aself * S.tiln;
    if (R.xh != 0.0) af *= fexp(R.xh * S.tiln);
    if (R.xhs != 0.0) as *= fexp(R.xhs * S.tiln);
    c1 = c1 + (af * entry(R.sh, field == MWRT_PAR_H2O_SH, all) + as * entry(R.shs, field == MWRT_PAR_H2O_SHS, all));
  }
  const double s1unit = (R.fl != 0.0) ? fdiv(1.0, R.fl * R.fl) : 0.0;                 // R.s1 = S1 / fl^2
  const du s = entry(R.s1, field == MWRT_PAR_H2O_S1, all, s1unit) *
               (S.ti2 * uexp((1.0 - S.ti) * entry(R.b2, field == MWRT_PAR_H2O_B2, all)));
  const du wsq = w0 * w0;
  const du base = udiv(w0, wsq + 562500.0);
  const du d1 = {f - c1.v, -c1.d}, d2 = {f + c1.v, c1.d};
  double w2 = 0.0;
  if (M->h2o_w2[k] > 0.0)
    w2 = M->h2o_w2[k] * S.pda * fexp(M->h2o_xw2[k] * S.tiln) + M->h2o_w2s[k] * S.pvap * fexp(M->h2o_xw2s[k] * S.tiln);
  const bool sd_in = w2 > 0.0 && fabs(d1.v) < 10.0 * w0.v;
  du term = {0.0, 0.0};
  if (fabs(d1.v) < 750.0 && !sd_in) term = term + (udiv(w0, d1 * d1 + wsq) - base);
  if (fabs(d2.v) < 750.0) term = term + (udiv(w0, d2 * d2 + wsq) - base);
  if (sd_in) {
    // Re SD and its tangent as k_absorb_tl forms them: Xc = A / B, A = w0 - 1.5 w2 + i (d1 + 1.5 delta2), B = w2 - i delta2;
    // no parameter offered here moves B, so dSD = CA dA, CA = -2 K h / B^2, K = sqrt(pi) (w + xrt w'), h = 1 / (2 xrt)
    const double dl2 = M->h2o_d2[k] * S.pda + M->h2o_d2s[k] * S.pvap;
    const cplx iB = crecip(cplx{w2, -dl2});
    const cplx xc = cmul(cplx{w0.v - 1.5 * w2, d1.v + 1.5 * dl2}, iB);
    const cplx xrt = csqrt_principal(xc);
    cplx w, dw;
    hui_w_dw(xrt, w, dw);
    const double SQPI = 1.77245385090551603;
    const cplx pxw = cmul(cscale(xrt, SQPI), w);
    const cplx sdc = cmul(cplx{2.0 - 2.0 * pxw.re, -2.0 * pxw.im}, iB);
    const cplx K = cscale(caddc(w, cmul(xrt, dw)), SQPI);
    const cplx h = crecip(cscale(xrt, 2.0));
    const cplx CA = cscale(cmul(cmul(K, h), cmul(iB, iB)), -2.0);
    term = term + du{sdc.re - base.v, re_mul(CA, cplx{w0.d, d1.d}) - base.d};
  }
  return s * term;
}

// the O2 quantities that carry a tangent under MWRT_PAR_O2_X (b = th^x; every other parameter leaves them plain values)
struct O2State { du den, ymul, pe2; double dens; };

__device__ __forceinline__ O2State o2_state(cmodel M, const Level& S, bool xhit) {
  const du b = {S.b, xhit ? S.b * S.lnth : 0.0};
  O2State Q;
  Q.den = 0.001 * (S.presda * b + (M->o2_wv_factor * S.preswv * S.th));
  Q.dens = 0.001 * ((S.presda + M->o2_wv_factor * S.preswv) * S.th);
  Q.ymul = (M->o2_mix_mode != 0) ? Q.den : (0.001 * S.P) * b;
  Q.pe2 = Q.den * Q.den;
  return Q;
}

// O2 line k's term of k_absorb_tl's `sum` (before 2 o2_coef presda th^3 f^2): (f^2 Pp + Qq) / (D1 D2)
__device__ __forceinline__ du o2_line(cmodel M, int k, int field, bool all, const Level& S, const O2State& Q, double f) {
  const auto& R = M->o2r[k];
  const bool second = M->o2_mix_mode != 0;
  const du y = Q.ymul * (S.th1 * entry(R.y1, field == MWRT_PAR_O2_Y1, all) + entry(R.y0, field == MWRT_PAR_O2_Y0, all));
  du dnu = {0.0, 0.0}, gfac = {1.0, 0.0};
  if (second) {
    dnu = Q.pe2 * (S.th1 * entry(R.dnu1, field == MWRT_PAR_O2_DNU1, all) + entry(R.dnu0, field == MWRT_PAR_O2_DNU0, all));
    gfac = 1.0 + Q.pe2 * (S.th1 * entry(R.g1, field == MWRT_PAR_O2_G1, all) + entry(R.g0, field == MWRT_PAR_O2_G0, all));
  }
  const bool line1_dens = !second && M->o2_line1_dens && k == 0;
  const du df = entry(R.w300, field == MWRT_PAR_O2_W300, all) * (line1_dens ? du{Q.dens, 0.0} : Q.den);
  const du str = entry(R.s300rf2, field == MWRT_PAR_O2_S300, all, M->o2_rf2[k]) *       // R.s300rf2 = S300 / F^2
                 uexp((-S.th1) * entry(R.be, field == MWRT_PAR_O2_BE, all));
  const du c1 = dnu + R.f;
  const du df2 = df * df;
  const du a = str * df * gfac;
  const du cb = c1 * (str * y);
  const du cc = c1 * c1 + df2;
  const du Pp = a + cb, Qq = cc * (a - cb);
  const du d1 = {f - c1.v, -c1.d}, d2 = {f + c1.v, c1.d};
  const du D1 = d1 * d1 + df2, D2 = d2 * d2 + df2;
  return udiv((f * f) * Pp + Qq, D1 * D2);
}

// the non-resonant term of the O2 bracket
__device__ __forceinline__ du o2_nonres(cmodel M, const Level& S, du dfnr, double f2) {
  return udiv((f2 * (0.5 * M->o2_nonres)) * dfnr, S.th * (dfnr * dfnr + f2));
}

// max(o2abs, 0) of this level and frequency clamps: every O2 parameter has zero slope there
__device__ __forceinline__ bool o2_clamped(cmodel M, const Level& S, double f) {
  const O2State Q = o2_state(M, S, false);
  double sum = 0.0;
  for (int k = 0; k < M->n_o2; ++k) sum += o2_line(M, k, -1, false, S, Q, f).v;
  const double f2 = f * f;
  const double o2 = f2 * sum + o2_nonres(M, S, du{M->o2_wb300 * Q.den.v, 0.0}, f2).v;   // (times a scale of the sign of presda)
  return !(((2.0 * M->o2_coef) * (S.presda * (S.th * S.th * S.th))) * o2 > 0.0);
}

// d alpha / d b of one level at one frequency [Np/km per unit of the entry]: alpha = awet for an H2O parameter, adry else.
// field and line are the same in every lane (scalar registers): the table reads are scalar loads.
__device__ __forceinline__ double dalpha(cmodel M, int field, int line, const Level& S, double f, bool clamped) {
  const double f2 = f * f;
  const bool all = line < 0;
  if (is_wet(field)) {
    if (field <= MWRT_PAR_H2O_XCS) {                       // the continuum: con0 = (cf pda ti^xcf + cs pvap ti^xcs) pvap
      const bool self = field == MWRT_PAR_H2O_CS || field == MWRT_PAR_H2O_XCS;
      const double x = self ? M->h2o_xcs : M->h2o_xcf, c = self ? M->h2o_cs : M->h2o_cf;
      const double pw = (self ? S.pvap : S.pda) * fexp(x * S.lnc) * S.pvap;
      return f2 * ((field == MWRT_PAR_H2O_CF || field == MWRT_PAR_H2O_CS) ? pw : c * pw * S.lnc);
    }
    if (M->h2o_shift_mode == 0 && (field == MWRT_PAR_H2O_SH || field == MWRT_PAR_H2O_SHS)) return 0.0;   // not read
    double acc = 0.0;
    if (all) for (int k = 0; k < M->n_h2o; ++k) acc += h2o_line(M, k, field, true, S, f).d;
    else acc = h2o_line(M, line, field, false, S, f).d;
    return f2 * ((3.183e-05 * M->h2o_den_coef) * S.rho) * acc;
  }
  if (field == MWRT_PAR_N2_L) {
    const double pn2 = M->n2_ptot ? S.P : S.pdry;
    double fdep = 1.0;
    if (M->n2_fdep) { const double qq = f * (1.0 / 450.0); fdep = 0.5 + fdiv(0.5, 1.0 + qq * qq); }
    return (fdep * f2) * (M->n2_n * (pn2 * pn2 * fexp(M->n2_m * S.lnth)));
  }
  if (clamped) return 0.0;
  const double scale2 = (2.0 * M->o2_coef) * (S.presda * (S.th * S.th * S.th));
  if (field == MWRT_PAR_O2_WB300) {
    const O2State Q = o2_state(M, S, false);
    return scale2 * o2_nonres(M, S, du{M->o2_wb300 * Q.den.v, Q.den.v}, f2).d;
  }
  if (field == MWRT_PAR_O2_X) {                            // b = th^x reaches every line through den (and Y, first order)
    const O2State Q = o2_state(M, S, true);
    double acc = 0.0;
    for (int k = 0; k < M->n_o2; ++k) acc += o2_line(M, k, -1, false, S, Q, f).d;
    return scale2 * (f2 * acc + o2_nonres(M, S, M->o2_wb300 * Q.den, f2).d);
  }
  if (M->o2_mix_mode == 0 && field >= MWRT_PAR_O2_G0) return 0.0;                      // G0, G1, DNU0, DNU1: not read
  const O2State Q = o2_state(M, S, false);
  double acc = 0.0;
  if (all) for (int k = 0; k < M->n_o2; ++k) acc += o2_line(M, k, field, true, S, Q, f).d;
  else acc = o2_line(M, line, field, false, S, Q, f).d;
  return scale2 * (f2 * acc);
}

// ---------------------------------------------------------------------------------------------
// k_par_tangent: one wave = 64 levels of one profile at one frequency; per parameter of the group one value per lane,
// stored as a row of consecutive levels (coalesced).  The register-hungry half (the speed-dependent shape's rational).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_par_tangent(const ParTangentArgs A) {
  const int lane = threadIdx.x;
  const int64_t pf = blockIdx.x / A.nslab;                               // profile * nf + frequency
  const int lev = (int)(blockIdx.x - pf * A.nslab) * WAVE + lane;
  const int64_t prof = pf / A.nf;
  const int j = (int)(pf - prof * A.nf);
  const bool live = lev < A.nlev;
  const cmodel M = (cmodel)A.M;
  const int64_t off = prof * A.nlev + (live ? lev : A.nlev - 1);
  const double f = ((cdoubles)A.frq)[j];
  const Level S = level_of(M, A.p[off], A.t[off], A.rh[off]);
  // one pass over the O2 lines, and only when an O2 parameter is in the group (the same in every workgroup)
  const bool clamped = A.o2_any ? o2_clamped(M, S, f) : false;
  double* out = A.dalpha + pf * A.gn * A.nlev + lev;
  for (int q = 0; q < A.gn; ++q) {
    const int field = __builtin_amdgcn_readfirstlane(A.params[A.p0 + q].field);
    const int line = __builtin_amdgcn_readfirstlane(A.params[A.p0 + q].line);
    const double v = dalpha(M, field, line, S, f, clamped);
    if (live) out[(int64_t)q * A.nlev] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// k_par_contract: one workgroup per (profile, frequency), one lane per level.  The layer rule, the Planck-space RTE and
// their adjoint are k_jac_rte's clear-sky statements, fed by k_absorb_tl's awet / adry; per elevation they give the level
// sensitivities s_wet, s_dry, parked in LDS rows for a chunk of elevations (each lane reads back its own entries).  Then
// every parameter's row is read once per chunk and summed against them over the levels: the lanes of a wave by a fixed
// shuffle tree, the waves in index order.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_par_contract(const ParContractArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, nthr = blockDim.x, nwaves = nthr / WAVE;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nlev = A.nlev, nf = A.nf, nang = A.nang, npar = A.npar, AC = A.achunk;
  const int64_t prof = blockIdx.x / nf;
  const int j = (int)(blockIdx.x - prof * nf);
  double* s0 = smem;
  double* s1 = smem + nthr;
  double* s2 = smem + 2 * nthr;
  double* wsum = smem + 3 * nthr;                  // 16 doubles
  double* red = smem + 3 * nthr + 16;              // [CONTRACT_PB][AC][nwaves]: the waves' partial sums of a block of parameters
  double* sens = red + CONTRACT_PB * AC * nwaves + tid;   // [AC][2][nthr]: s_wet, s_dry of the chunk's elevations
  const cmodel M = (cmodel)A.M;
  const bool live = tid < nlev;
  const int l = live ? tid : nlev - 1;
  const int64_t lo = prof * nlev + l, ao = (prof * nf + j) * nlev + l;
  const double qnan = __builtin_nan("");
  const bool first = A.p0 == 0;                     // the first group's launch also writes valid and the TBs

  const double zl = A.z[lo], tl = A.t[lo];
  const unsigned fl = A.flags[prof];                // a NaN in p, T or rh, or a negative absorption: from k_absorb_tl
  const bool bad_nan = __syncthreads_or(live && (isnan(zl) || isnan(tl))) || (fl & 1u);
  const bool bad = bad_nan || (fl & 2u);
  if (first && j == 0 && tid == 0) A.valid[prof] = bad_nan ? 0 : (bad ? 2 : 1);
  if (bad) {                           // NaN in the profile (0) or negative absorption (2): the whole profile is NaN
    for (int a = 0; a < nang; ++a) {
      const int64_t row = (prof * nang + a) * nf + j;
      for (int q = tid; q < A.gn; q += nthr) A.dtb_db[row * npar + A.p0 + q] = qnan;
      if (first && tid == 0 && A.tb) A.tb[row] = qnan;
    }
    return;
  }
  const bool lay = live && tid > 0;
  const bool has_up = tid + 1 < nlev;
  const double aw = A.awet[ao], ad = A.adry[ao];
  const double hvk = A.frq[j] * (1e9 * M->planck_h / M->boltzmann_k);
  const double x = fdiv(hvk, tl);
  const double b = planck_b(x, fdiv(tl, hvk));

  // ---- per frequency: layer l (between levels l-1 and l) lives on lane l ----
  s0[tid] = aw; s1[tid] = ad; s2[tid] = b;
  __syncthreads();
  double Lw = 0.0, w1 = 0.0, w0 = 0.0, Ld = 0.0, d1 = 0.0, d0 = 0.0, dz = 0.0, bm = 0.0;
  if (lay) {
    bool neg = false;                  // (negative values are flagged by k_absorb_tl already)
    Lw = layer_value_tl(aw, s0[tid - 1], w1, w0, neg);
    Ld = layer_value_tl(ad, s1[tid - 1], d1, d0, neg);
    const double z0 = A.z[prof * nlev];
    dz = (zl - z0) - (A.z[lo - 1] - z0);
    bm = s2[tid - 1];
  }
  const double tauz = lay ? Lw * dz + Ld * dz : 0.0;                   // zenith optical depth of layer l
  __syncthreads();
  s0[tid] = w0; s1[tid] = d0;          // the lower-end partials of layer l, for level l-1
  __syncthreads();
  const double w0n = has_up ? s0[tid + 1] : 0.0, d0n = has_up ? s1[tid + 1] : 0.0;
  double tau_tot;
  const double cum_in = block_scan(tauz, wsum, tid, nwaves, tau_tot);
  const double cum_ex = cum_in - tauz;                                   // zenith optical depth below layer l
  const double bbg = fdiv(1.0, fexp(fdiv(hvk, M->t_cosmic)) - 1.0);
  const double* dal = A.dalpha + (prof * nf + j) * A.gn * nlev + l;     // this lane's level of every parameter row

  for (int a0 = 0; a0 < nang; a0 += AC) {
    const int an = min(AC, nang - a0);
    unsigned long long blank = 0ull;   // the chunk's NaN elevations (MWRT_MAX_ANGLES = 64 bits)
    // ---- the chunk's level sensitivities ----
    for (int c = 0; c < an; ++c) {
      const double am = A.airmass[a0 + c];
      const int64_t row = (prof * nang + a0 + c) * nf + j;
      if (isnan(am)) {                 // a NaN elevation: its rows are NaN, the profile stays valid
        blank |= 1ull << c;
        if (first && tid == 0 && A.tb) A.tb[row] = qnan;
        continue;
      }
      const double tau = am * tauz;
      const double E = fexp(-tau);
      const double th = (tau <= EXP_SMALL_X) ? ftanh_half_small(tau) : fdiv(1.0 - E, 1.0 + E);   // (1 - E) / (1 + E)
      const double Tm1 = fexp(-am * cum_ex);                               // transmittance below layer l
      const double Pc = lay ? (bm + b * E) * th * Tm1 : 0.0;
      double Bsum;
      (void)block_scan(Pc, wsum, tid, nwaves, Bsum);
      const double Ttop = fexp(-am * tau_tot);
      const double Btot = (Ttop > TRANS_MIN) ? __builtin_fma(bbg, Ttop, Bsum) : Bsum;
      // radiance reaching the antenna from above layer l, summed directly (B_tot - S_l would cancel where it is tiny)
      const double above = block_suffix_excl(Pc, wsum, tid, nwaves) + ((Ttop > TRANS_MIN) ? bbg * Ttop : 0.0);
      const double Lg = flog(1.0 + fdiv(1.0, Btot));
      const double dTB_dB = fdiv(hvk, Lg * Lg * Btot * (Btot + 1.0));
      const double opE = 1.0 + E;
      const double dc_dtau = fdiv(E * (2.0 * bm + 2.0 * b * E - b + b * E * E), opE * opE);
      const double g = lay ? dTB_dB * (Tm1 * dc_dtau - above) : 0.0;       // dTB / dtau_l (everything above l is dimmed)
      const double gk = g * am * dz;
      s0[tid] = gk;                    // (the scans' barriers lie between this and the previous elevation's reads)
      __syncthreads();
      const double gkn = has_up ? s0[tid + 1] : 0.0;
      // d TB / d alpha of level l: as the upper end of layer l and as the lower end of layer l + 1
      sens[(2 * c) * nthr] = live ? gk * w1 + gkn * w0n : 0.0;
      sens[(2 * c + 1) * nthr] = live ? gk * d1 + gkn * d0n : 0.0;
      if (first && tid == 0 && A.tb) A.tb[row] = fdiv(hvk, Lg);
    }
    // ---- the sums over the levels, CONTRACT_PB parameters at a time ----
    for (int q0 = 0; q0 < A.gn; q0 += CONTRACT_PB) {
      const int qn = min(CONTRACT_PB, A.gn - q0);
      for (int q = 0; q < qn; ++q) {
        const int field = __builtin_amdgcn_readfirstlane(A.params[A.p0 + q0 + q].field);
        const double da = live ? dal[(int64_t)(q0 + q) * nlev] : 0.0;
        const int sp = is_wet(field) ? 0 : 1;
        for (int c = 0; c < an; ++c) {
          double v = da * sens[(2 * c + sp) * nthr];
#pragma unroll
          for (int o = WAVE / 2; o >= 1; o >>= 1) v += __shfl_down(v, o, WAVE);    // a fixed tree: lane 0 holds the wave's sum
          if (lane == 0) red[(q * AC + c) * nwaves + wave] = v;
        }
      }
      __syncthreads();
      for (int i = tid; i < qn * an; i += nthr) {   // the waves in index order; consecutive lanes store consecutive parameters
        const int c = i / qn, q = i - c * qn;
        double acc = 0.0;
        for (int w = 0; w < nwaves; ++w) acc += red[(q * AC + c) * nwaves + w];
        const int64_t row = (prof * nang + a0 + c) * nf + j;
        A.dtb_db[row * npar + A.p0 + q0 + q] = ((blank >> c) & 1ull) ? qnan : acc;
      }
      __syncthreads();                 // red is written again by the next block
    }
  }
}

}  // namespace

hipError_t launch_par_tangent(const ParTangentArgs& a, int64_t nprof, hipStream_t st) {
  hipLaunchKernelGGL(k_par_tangent, dim3((unsigned)(nprof * a.nf * a.nslab)), dim3(WAVE), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_par_contract(ParContractArgs a, int64_t nprof, hipStream_t st) {
  const int threads = ((a.nlev + WAVE - 1) / WAVE) * WAVE;
  const int nwaves = threads / WAVE;
  int ac = CONTRACT_SENS_BYTES / (int)(2 * sizeof(double) * threads);
  ac = ac < 1 ? 1 : ac;
  a.achunk = ac < a.nang ? ac : a.nang;
  // 3 rows + the scans' 16 + the partial sums + the chunk's sensitivities: 21 KiB at 180 levels, 42 KiB at 1024
  const size_t lds = sizeof(double) * ((size_t)3 * threads + 16 + (size_t)CONTRACT_PB * a.achunk * nwaves +
                                       (size_t)2 * a.achunk * threads);
  hipLaunchKernelGGL(k_par_contract, dim3((unsigned)(nprof * a.nf)), dim3(threads), lds, st, a);
  return hipGetLastError();
}

}  // namespace par
}  // namespace mwrt
