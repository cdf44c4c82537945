// mwrt_tl_rte.hip.h -- the adjoint RTE of the device K-matrix as one __device__ body, shared by its two kernels:
// k_jac_rte (csrc/mwrt_tl.hip; one air mass per elevation, RAY = false) and ray::k_jac_rte_ray (csrc/mwrt_ray.hip; a path
// factor per (elevation, layer) and the response of that factor to the state, RAY = true).  Everything is
// __forceinline__, and every ray term sits behind `if constexpr (RAY)`: the plane-parallel kernel compiles to the code it
// had when the body stood in mwrt_tl.hip.  The mathematics: DESIGN.md sections 4.5 - 4.5.4.
#pragma once
#include "mwrt_tl.hip.h"
#include "mwrt_absorption.hip.h"      // level_state, goff_gratch_e, clog_, CLOUD_KICE (and the arithmetic of mwrt_math.hip.h)
#include "mwrt_tl_dev.hip.h"          // layer_value_tl, the workgroup scans

namespace mwrt {

// nothing is scheduled across this point (keeps independent chains from being interleaved where that costs registers)
#define MWRT_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// Cloud liquid absorption per unit water content and its exact T-derivative: kap = liquid_abs(cloud_level(M, tk), f, 1)
// [Np/km per g m-3] as the forward kernels compute it, kapT = d kap / dT of those formulas (both liq_modes).  The complex
// logarithms' values are clog_'s; their derivatives are quotients (d log w = dw / w), so nothing here differentiates atan2.
__device__ __forceinline__ void liquid_abs_tl(cmodel M, double tk, double f, double& kap, double& kapT) {
  cplx eps, deps;
  if (M->liq_mode == 0) {
    const double eps2 = 3.52;
    const double thr = fdiv(300.0, tk), theta1 = 1.0 - thr, dth = fdiv(thr, tk);
    const double eps0 = 77.66 - 103.3 * theta1, deps0 = -103.3 * dth;
    const double a = 0.0671 * eps0, da = 0.0671 * deps0;
    const double fp = (316.0 * theta1 + 146.4) * theta1 + 20.2, dfp = (632.0 * theta1 + 146.4) * dth;
    const double b = fdiv(1.0, fp), db = -dfp * b * b;
    const double c = fdiv(1.0, 39.8 * fp), dc = -39.8 * dfp * c * c;
    // t = A r, r = 1 / (1 + i f b):  dt = dA r - t r (i f db)
    const cplx r1 = crecip(cplx{1.0, f * b}), r2 = crecip(cplx{1.0, f * c});
    const cplx t1 = cscale(r1, eps0 - a), t2 = cscale(r2, a - eps2);
    const cplx dt1 = csub(cscale(r1, deps0 - da), cmul(cmul(t1, r1), cplx{0.0, f * db}));
    const cplx dt2 = csub(cscale(r2, da), cmul(cmul(t2, r2), cplx{0.0, f * dc}));
    eps = cplx{t1.re + t2.re + eps2, t1.im + t2.im};
    deps = caddc(dt1, dt2);
  } else {
    const double tc = tk - 273.15;
    const double lth = flog(fdiv(300.0, tk)), dlth = -fdiv(1.0, tk);
    const double e1 = -43.7527 * fexp(0.05 * lth), e2 = 299.504 * fexp(1.47 * lth), e3 = -399.364 * fexp(2.11 * lth),
                 e4 = 221.327 * fexp(2.31 * lth);
    const double eps0 = e1 + e2 + e3 + e4;
    const double deps0 = (0.05 * e1 + 1.47 * e2 + 2.11 * e3 + 2.31 * e4) * dlth;
    const double a = 80.69715 * fexp(-tc * (1.0 / 226.45)), da = -a * (1.0 / 226.45);                // delta
    const double qs = fdiv(1.0, tc + 133.07);
    const double b = 1164.023 * fexp(fdiv(-651.4728, tc + 133.07)), db = b * 651.4728 * qs * qs;      // sd
    const double c = 4.008724 * fexp(-tc * (1.0 / 103.05)), dc = -c * (1.0 / 103.05);                // delta_B
    const double f1 = 10.46012 + tc * (0.1454962 + tc * (0.063267156 + tc * 0.00093786645));
    const double df1 = 0.1454962 + tc * (2.0 * 0.063267156 + tc * (3.0 * 0.00093786645));
    const cplx z1 = {-0.75 * f1, f1}, dz1 = {-0.75 * df1, df1};
    // cnorm = log(z2 / z1), z1 = (-0.75 + i) f1:  d cnorm = -df1 / f1 (real), d (1 / cnorm) = (df1 / f1) / cnorm^2
    // (the three complex logarithms one after the other: interleaved, their atan2 chains would set the kernel's register count)
    const cplx icn = crecip(clog_(cdiv(cplx{-4500.0, 2000.0}, z1)));
    MWRT_SCHED_FENCE();
    const cplx dicn = cscale(cmul(icn, icn), fdiv(df1, f1));
    const cplx icj = {icn.re, -icn.im}, dicj = {dicn.re, -dicn.im};
    // kap0 = -delta z / (sd + z), z = i f
    const cplx rb = crecip(cplx{b, f});
    const cplx kap0 = cmul(cplx{0.0, -a * f}, rb);
    const cplx dkap0 = csub(cmul(cplx{0.0, -da * f}, rb), cscale(cmul(kap0, rb), db));
    // log((z - z2) / (z - z1)) and its conjugate-pole twin: d log = dz1 / (z - z1)
    const cplx zp = {-z1.re, f - z1.im}, zj = {-z1.re, f + z1.im};
    const cplx lp = clog_(cdiv(cplx{4500.0, f - 2000.0}, zp));
    MWRT_SCHED_FENCE();
    const cplx lj = clog_(cdiv(cplx{4500.0, f + 2000.0}, zj));
    MWRT_SCHED_FENCE();
    const cplx dlp = cdiv(dz1, zp), dlj = cdiv(cplx{dz1.re, -dz1.im}, zj);
    const double hd = 0.5 * c, dhd = 0.5 * dc;
    const cplx hlp = cscale(lp, hd), hlj = cscale(lj, hd);
    const cplx chip = cmul(hlp, icn), chij = cmul(hlj, icj);
    const cplx dchip = caddc(cmul(caddc(cscale(lp, dhd), cscale(dlp, hd)), icn), cmul(hlp, dicn));
    const cplx dchij = caddc(cmul(caddc(cscale(lj, dhd), cscale(dlj, hd)), icj), cmul(hlj, dicj));
    eps = cplx{eps0 + (kap0.re + (chip.re + chij.re - c)), kap0.im + (chip.im + chij.im)};
    deps = cplx{deps0 + (dkap0.re + (dchip.re + dchij.re - dc)), dkap0.im + (dchip.im + dchij.im)};
  }
  // re = (eps - 1) / (eps + 2):  d re = 3 d eps / (eps + 2)^2
  const cplx ie2 = crecip(cplx{eps.re + 2.0, eps.im});
  const cplx re = cmul(cplx{eps.re - 1.0, eps.im}, ie2);
  const cplx dre = cscale(cmul(deps, cmul(ie2, ie2)), 3.0);
  kap = -0.06286 * re.im * f;
  kapT = -0.06286 * dre.im * f;
}
#undef MWRT_SCHED_FENCE

// Goff-Gratch saturation vapour pressure over water and its T-derivative, in goff_gratch_e's own form:
// es = 10^g(y), y = 373.16 / T, so d es / dT = es ln10 g'(y) (-y / T)
__device__ __forceinline__ void goff_gratch_es_tl(double tk, double& es, double& des) {
  const double LN10 = 2.302585092994045684;
  const double INV_LN10 = 0.434294481903251828;
  const double y = 373.16 / tk;
  const double a = fexp(LN10 * (11.344 * (1.0 - (1.0 / y)))), b = fexp(LN10 * (-3.49149 * (y - 1.0)));
  const double g = -7.90298 * (y - 1.0) + 5.02808 * (flog(y) * INV_LN10) - 1.3816e-07 * (a - 1.0) + 0.0081328 * (b - 1.0) +
                   3.0057148979490314 /*log10(1013.246)*/;
  const double gy = -7.90298 + fdiv(5.02808 * INV_LN10, y) - (1.3816e-07 * 11.344 * LN10) * fdiv(a, y * y) -
                    (0.0081328 * 3.49149 * LN10) * b;
  es = fexp(LN10 * g);
  des = es * LN10 * gy * -fdiv(y, tk);
}

// The partial derivatives of thayer_refindex(p, T, e) with respect to T (at fixed e and p) and e (at fixed T and p),
// differentiated by hand from that function's own statements
__device__ __forceinline__ void thayer_refindex_tl(double p, double tk, double e, double& dn_dt, double& dn_de) {
  const double pa = p - e, tc = tk - 273.16, tc2 = tc * tc, itk = 1.0 / tk, itk2 = itk * itk;
  const double A = 5.79e-07 * (1.0 + 0.52 * itk) - (0.00094611 * tc) * itk2;
  const double At = -5.79e-07 * 0.52 * itk2 - 0.00094611 * (itk2 - 2.0 * tc * itk2 * itk);
  const double rza = 1.0 + pa * A;
  const double B = 1.0 - 0.01317 * tc + 0.000175 * tc2 + 1.44e-06 * (tc2 * tc);
  const double Bt = -0.01317 + 0.00035 * tc + 4.32e-06 * tc2;
  const double it3 = itk * itk2;
  const double rzw = 1.0 + 1650.0 * (e * it3) * B;
  const double rzw_e = 1650.0 * it3 * B, rzw_t = 1650.0 * e * (Bt * it3 - 3.0 * B * it3 * itk);
  const double W = 64.79 * (e * itk) + 377600.0 * (e * itk2);
  const double W_e = 64.79 * itk + 377600.0 * itk2, W_t = -64.79 * e * itk2 - 2.0 * 377600.0 * e * it3;
  const double dry_e = 77.6036 * (-itk * rza - (pa * itk) * A);
  const double dry_t = 77.6036 * (-pa * itk2 * rza + (pa * itk) * (pa * At));
  dn_de = (dry_e + (W_e * rzw + W * rzw_e)) * 1e-06;
  dn_dt = (dry_t + (W_t * rzw + W * rzw_t)) * 1e-06;
}

// ---------------------------------------------------------------------------------------------
// The adjoint RTE: one workgroup per (profile, frequency), one lane per level.  Per frequency the layer values, their partial
// derivatives, the Planck terms and the zenith optical-depth prefix are formed once; per elevation the transmittances,
// one workgroup prefix sum (S_l = sum_{m <= l} c_m T_{m-1}) and a neighbour exchange give every level's three
// derivatives, which the lanes store as one contiguous row (level fastest: coalesced).
//
// RAY: the slant optical depth of layer l is path[0][l] tauz_l instead of airmass tauz_l, `path` being the six
// rows of ray::k_ray_paths_tl per (profile, elevation): the factor f and its partials towards n_l, n_{l-1}, n_0 (the
// refractive index of the layer's two ends and of the ground) and towards the relative heights z_l, z_{l-1} of its ends.
// The transmittance below a layer then takes a prefix sum per elevation, and with q_l = dTB/dtau_l tauz_l the rows gain
//   level l >= 0:  (q_l df_l/dn_l + q_{l+1} df_{l+1}/dn_l) dn_l/d(T, e)          neighbour exchange
//   level 0:       (sum_l q_l df_l/dn_0) dn_0/d(T, e)                            one workgroup sum, fixed order
//   thickness i:   q_i df_i/dz_i + sum_{l > i} q_l (df_l/dz_l + df_l/dz_{l-1})   one suffix sum, fixed order
// before the change of variables.  `duct` [nprof]: a ray of the profile was trapped (valid = 3).
// ---------------------------------------------------------------------------------------------
template <bool RAY>
__device__ __forceinline__ void jac_rte_body(const JacRteArgs& A, const double* __restrict__ path,
                                             const uint8_t* __restrict__ duct) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, nthr = blockDim.x, nwaves = nthr / WAVE;
  const int nlev = A.nlev, nf = A.nf, nang = A.nang;
  const int64_t prof = blockIdx.x / nf;
  const int j = (int)(blockIdx.x - prof * nf);
  double* s0 = smem;
  double* s1 = smem + nthr;
  double* s2 = smem + 2 * nthr;
  double* wsum = smem + 3 * nthr;
  const cmodel M = (cmodel)A.M;
  const bool live = tid < nlev;
  const int l = live ? tid : nlev - 1;
  const int64_t lo = prof * nlev + l, ao = (prof * nf + j) * nlev + l;
  const double qnan = __builtin_nan("");

  const double zl = A.z[lo], tl = A.t[lo];
  const unsigned fl = A.flags[prof];
  // cloud liquid / ice: every branch on it is uniform across the workgroup, and a call without cloud
  // arrays executes the clear-sky arithmetic alone
  const bool cloud_call = A.denliq != nullptr || A.denice != nullptr;
  double denl = 0.0, deni = 0.0;
  bool nan_here = live && (isnan(zl) || isnan(tl));
  if (cloud_call) {
    if (A.denliq) denl = A.denliq[lo];
    if (A.denice) deni = A.denice[lo];
    nan_here = nan_here || (live && (isnan(denl) || isnan(deni)));
  }
  const bool bad_nan = __syncthreads_or(nan_here) || (fl & 1u);
  const bool bad = bad_nan || (fl & 2u);
  // a cloudy call's valid array is preset to 1 by the entry point and only ever lowered here (the cloud terms are
  // checked per frequency, further down); a clear call writes all three values
  if (j == 0 && tid == 0 && (bad || !cloud_call)) A.valid[prof] = bad_nan ? 0 : (bad ? 2 : 1);
  auto blank_profile = [&]() {
    for (int a = 0; a < nang; ++a) {
      const int64_t row = (prof * nang + a) * nf + j;
      if (live) {
        A.dtb_dt[row * nlev + tid] = qnan; A.dtb_de[row * nlev + tid] = qnan;
        if (A.dtb_ddz) A.dtb_ddz[row * nlev + tid] = qnan;
        if (A.dtb_dliq) A.dtb_dliq[row * nlev + tid] = qnan;
        if (A.dtb_dice) A.dtb_dice[row * nlev + tid] = qnan;
      }
      if (tid == 0) A.tb[row] = qnan;
    }
  };
  if (bad) {                           // NaN in the profile (0) or negative absorption (2): the whole profile is NaN
    blank_profile();
    return;
  }
  // skipped for a profile that holds no cloud at all (workgroup vote), as in the forward kernel
  const bool cloudy = cloud_call && __syncthreads_or(live && (denl > 0.0 || deni > 0.0));
  // ---- cloud: aliq = denl kap(T, f) (denl > 0, else 0), aice = CLOUD_KICE f deni (deni > 0, else 0), the zeroflg = false
  // layer rule and the neighbour exchange through the LDS rows, before the clear-sky operands are loaded (few registers
  // are live here).  What the elevation loop needs per level goes to seven LDS rows of a cloudy launch, each lane reading
  // back its own entries, so the loop holds no more registers than the clear one:
  //   Lc = Ll + Li;  ql1, ql0 = the partials of layers l and l+1 towards aliq_l, times kap (d aliq / d denl);
  //   tl1, tl0 the same times denl dkap/dT (d aliq / dT);  qi1, qi0 those of the ice layers times d aice / d deni
  const bool lay = live && tid > 0;
  const bool has_up = tid + 1 < nlev;
  double* cst = smem + 3 * nthr + 16 + tid;
  double tci = 0.0, tli = 0.0;         // ice and liquid zenith optical depth of layer l
  if (cloudy) {
    double kap = 0.0, kapT = 0.0;
    if (denl > 0.0) liquid_abs_tl(M, tl, A.frq[j], kap, kapT);
    const double kice = (deni > 0.0) ? CLOUD_KICE * A.frq[j] : 0.0;
    const double al = kap * denl, ai = kice * deni;
    s0[tid] = al; s1[tid] = ai;
    __syncthreads();
    double Ll = 0.0, l1 = 0.0, l0 = 0.0, Li = 0.0, i1 = 0.0, i0 = 0.0;
    bool neg = false;
    if (lay) {
      Ll = layer_value_tl<false>(al, s0[tid - 1], l1, l0, neg);
      Li = layer_value_tl<false>(ai, s1[tid - 1], i1, i0, neg);
      const double z0 = A.z[prof * nlev];
      const double dzc = (zl - z0) - (A.z[lo - 1] - z0);
      tci = Li * dzc; tli = Ll * dzc;
    }
    if (__syncthreads_or(neg)) {       // a negative cloud coefficient: flag 2 (the rows of this frequency are NaN)
      if (tid == 0) A.valid[prof] = 2;
      blank_profile();
      return;
    }
    s0[tid] = l0; s1[tid] = i0;
    __syncthreads();
    const double l0n = has_up ? s0[tid + 1] : 0.0, i0n = has_up ? s1[tid + 1] : 0.0;
    cst[0] = Ll + Li;
    cst[nthr] = l1 * kap; cst[2 * nthr] = l0n * kap;
    cst[3 * nthr] = l1 * (denl * kapT); cst[4 * nthr] = l0n * (denl * kapT);
    cst[5 * nthr] = i1 * kice; cst[6 * nthr] = i0n * kice;
    __syncthreads();                   // s0 / s1 are about to hold the clear-sky rows
  }
  // ---- retrieval variables: the per-level factors of the change of variables, formed once and parked in
  // nine LDS rows behind the cloud rows, each lane reading back its own entries inside the elevation loop.  Every branch
  // on a mode is uniform across the workgroup, and a call with all three modes 0 executes none of this.
  //   hydrostatic heights: dz_l = c_l (Tv_l + Tv_{l-1}), c_l = (287.04 / (2 g)) ln(p_{l-1} / p_l) / 1000 (c_0 = 0), so the
  //   thickness rows Z_l and Z_{l+1} reach level l through kT = dTv/dT|e = 1 + 0.608 q and kE = dTv/de|T =
  //   0.608 T 0.622 p / (p - 0.378 e)^2, q = 0.622 e / (p - 0.378 e):  v0 = c_l kT, v1 = c_{l+1} kT, v2 = c_l kE, v3 = c_{l+1} kE
  //   humidity h: v4 = de/dh (es(T) for rh, p / 1e6 for ppmv), v5 = de/dT at fixed h (rh es'(T) for rh, else 0)
  //   cloud as kg/kg: v6 = 1000 rho_air = 1e5 p / (287.06 T), v7 = denliq / T, v8 = denice / T
  const bool vars_call = (A.humidity | A.cloud | A.heights) != 0;
  double* vst = smem + (cloud_call ? 10 : 3) * nthr + 16 + tid;
  if (vars_call) {
    const double pl = A.p[lo], rhl = A.rh[lo];
    double es = 0.0, des = 0.0;
    if (A.heights || A.humidity == 1) goff_gratch_es_tl(tl, es, des);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (A.heights) {
      const double e = rhl * es, ipe = fdiv(1.0, pl - 0.378 * e);
      const double kT = 1.0 + 0.608 * (0.622 * e * ipe), kE = 0.608 * tl * (0.622 * pl) * (ipe * ipe);
      const double RG = 287.04 / (2.0 * 9.80665) / 1000.0;
      const double cl = lay ? RG * flog(fdiv(A.p[lo - 1], pl)) : 0.0;
      const double cn = has_up ? RG * flog(fdiv(pl, A.p[lo + 1])) : 0.0;
      v[0] = cl * kT; v[1] = cn * kT; v[2] = cl * kE; v[3] = cn * kE;
    }
    vst[0] = v[0]; vst[nthr] = v[1]; vst[2 * nthr] = v[2]; vst[3 * nthr] = v[3];
    vst[4 * nthr] = (A.humidity == 1) ? es : (A.humidity == 2) ? pl * 1e-6 : 1.0;
    vst[5 * nthr] = (A.humidity == 1) ? rhl * des : 0.0;
    const double it = fdiv(1.0, tl);
    vst[6 * nthr] = (1e5 / 287.06) * pl * it;
    vst[7 * nthr] = denl * it; vst[8 * nthr] = deni * it;
  }
  // ---- ray paths: the level's d n / dT at fixed e and d n / de at fixed T; the path terms change lanes by a
  // shuffle, the wave seams through 3 x 16 doubles behind every row (a launch at 1024 levels has no LDS row to spare)
  double* seam = smem + ((cloud_call ? 10 : 3) + (vars_call ? JAC_VARS_ROWS : 0)) * nthr + 16;
  double nT = 0.0, nE = 0.0;
  if constexpr (RAY) thayer_refindex_tl(A.p[lo], tl, goff_gratch_e(tl, A.rh[lo]), nT, nE);
  const double aw = A.awet[ao], ad = A.adry[ao];
  const double awT = A.dawet_dt[ao], awE = A.dawet_de[ao], adT = A.dadry_dt[ao], adE = A.dadry_de[ao];
  const double hvk = A.frq[j] * (1e9 * M->planck_h / M->boltzmann_k);
  const double x = fdiv(hvk, tl);
  const double b = planck_b(x, fdiv(tl, hvk));
  const double dbdT = fdiv(b * (b + 1.0) * x, tl);                       // db/dT = b (b + 1) hvk / T^2

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
  double bnx = b;                      // RAY: the Planck term of the level above (the top level: its own)
  if constexpr (RAY) { if (has_up) bnx = s2[tid + 1]; }
  double tauz = lay ? Lw * dz + Ld * dz : 0.0;                         // zenith optical depth of layer l
  __syncthreads();
  s0[tid] = w0; s1[tid] = d0;          // the lower-end partials of layer l, for level l-1
  __syncthreads();
  const double w0n = has_up ? s0[tid + 1] : 0.0, d0n = has_up ? s1[tid + 1] : 0.0;
  if (cloudy) tauz = (tauz + tci) + tli;                              // the forward's order: ((wet + dry) + ice) + liquid
  double tau_tot = 0.0, cum_ex = 0.0;
  if constexpr (!RAY) {
    const double cum_in = block_scan(tauz, wsum, tid, nwaves, tau_tot);
    cum_ex = cum_in - tauz;                                              // zenith optical depth below layer l
  }
  const double bbg = fdiv(1.0, fexp(fdiv(hvk, M->t_cosmic)) - 1.0);

  for (int a = 0; a < nang; ++a) {
    double am;
    const double* fr = nullptr;        // RAY: this lane's entry of the six path rows of (profile, elevation)
    const int64_t row = (prof * nang + a) * nf + j;
    double* o_t = A.dtb_dt + row * nlev;
    double* o_e = A.dtb_de + row * nlev;
    double* o_z = A.dtb_ddz ? A.dtb_ddz + row * nlev : nullptr;
    double* o_l = A.dtb_dliq ? A.dtb_dliq + row * nlev : nullptr;
    double* o_i = A.dtb_dice ? A.dtb_dice + row * nlev : nullptr;
    bool blank;
    if constexpr (RAY) {
      fr = path + (prof * nang + a) * (6 * (int64_t)nlev) + l;
      am = fr[0];                      // the layer's own path factor ds / dz
      // a NaN elevation or a trapped ray: every factor above the ground is NaN
      blank = __syncthreads_or(live && isnan(am));
    } else {
      am = A.airmass[a];
      blank = isnan(am);
    }
    if (blank) {                       // a NaN elevation: its rows are NaN, the profile stays valid
      if (live) { o_t[tid] = qnan; o_e[tid] = qnan; if (o_z) o_z[tid] = qnan; if (o_l) o_l[tid] = qnan; if (o_i) o_i[tid] = qnan; }
      if (tid == 0) A.tb[row] = qnan;
      continue;
    }
    const double tau = am * tauz;
    if constexpr (RAY) {               // the slant optical depth below layer l: a prefix sum per elevation
      const double cum_in = block_scan(tau, wsum, tid, nwaves, tau_tot);
      cum_ex = cum_in - tau;
    }
    const double E = fexp(-tau);
    const double th = (tau <= EXP_SMALL_X) ? ftanh_half_small(tau) : fdiv(1.0 - E, 1.0 + E);   // (1 - E) / (1 + E)
    const double Tm1 = RAY ? fexp(-cum_ex) : fexp(-am * cum_ex);         // transmittance below layer l
    const double Tl = Tm1 * E;
    const double Pc = lay ? (bm + b * E) * th * Tm1 : 0.0;
    double Bsum;
    (void)block_scan(Pc, wsum, tid, nwaves, Bsum);
    const double Ttop = RAY ? fexp(-tau_tot) : fexp(-am * tau_tot);
    const double Btot = (Ttop > TRANS_MIN) ? __builtin_fma(bbg, Ttop, Bsum) : Bsum;
    // radiance reaching the antenna from above layer l (sum_{m > l} c_m T_{m-1} + the cosmic term), summed directly:
    // B_tot - S_l would cancel to ~eps B_tot where it is tiny
    const double above = block_suffix_excl(Pc, wsum, tid, nwaves) + ((Ttop > TRANS_MIN) ? bbg * Ttop : 0.0);
    const double Lg = flog(1.0 + fdiv(1.0, Btot));
    const double dTB_dB = fdiv(hvk, Lg * Lg * Btot * (Btot + 1.0));
    const double opE = 1.0 + E;
    const double dc_dtau = fdiv(E * (2.0 * bm + 2.0 * b * E - b + b * E * E), opE * opE);
    double g = 0.0;                                                      // dTB / dtau_l (everything above l is dimmed)
    if constexpr (RAY) {
      // The same quantity with the first layer above taken out of `above` and joined to the layer's own term:
      //   Tm1 dc/dtau - above = 2 Tm1 E (bm - b) / (1 + E)^2 + [ T_l E' (2 b - b' + b' E') / (1 + E') - above' ],
      // E', b', above' those of lane l+1.  Below an opaque layer that starts at the same temperature the two terms of the
      // plain form agree to seven digits (the layer's emission is absorbed at once): measured 2.5e-8 of a row at 60.3 GHz
      // and 4.2 degrees on a repeated level; this form has no such difference left.
      const double cosmic = (Ttop > TRANS_MIN) ? bbg * Ttop : 0.0;
      double En = __shfl_down(E, 1, WAVE), an = __shfl_down(above, 1, WAVE);
      if ((tid & (WAVE - 1)) == 0) { seam[16 + tid / WAVE] = E; seam[32 + tid / WAVE] = above; }
      __syncthreads();
      if ((tid & (WAVE - 1)) == WAVE - 1 && has_up) { En = seam[16 + tid / WAVE + 1]; an = seam[32 + tid / WAVE + 1]; }
      if (!has_up) { En = 1.0; an = cosmic; }
      const double own = fdiv(2.0 * Tm1 * E * (bm - b), opE * opE);
      const double next = fdiv(Tl * En * (2.0 * b - bnx + bnx * En), 1.0 + En);
      g = lay ? dTB_dB * (own + (next - an)) : 0.0;
    } else {
      g = lay ? dTB_dB * (Tm1 * dc_dtau - above) : 0.0;
    }
    const double gk = g * am * dz;
    // dTB / d(thickness of layer l) [K/km]: tau_l = m (Lw + Ld + Ll + Li) dz_l is linear in dz_l, so this holds at
    // dz_l = 0 too
    double zr = lay ? g * am * (cloudy ? (Lw + Ld) + cst[0] : Lw + Ld) : 0.0;
    double pn = 0.0, pnn = 0.0;        // RAY: dTB / dn_l through the path factors of layers l and l+1
    if constexpr (RAY) {
      const double q = g * tauz;
      double n0sum;
      (void)block_scan(q * fr[3 * (int64_t)nlev], wsum, tid, nwaves, n0sum);
      const double zq = q * (fr[4 * (int64_t)nlev] + fr[5 * (int64_t)nlev]);
      const double zabove = block_suffix_excl(zq, wsum, tid, nwaves);
      zr = lay ? zr + (q * fr[4 * (int64_t)nlev] + zabove) : 0.0;
      pn = q * fr[(int64_t)nlev] + (tid == 0 ? n0sum : 0.0);
      const double qlow = q * fr[2 * (int64_t)nlev];                     // layer l towards its lower end: for level l-1
      pnn = __shfl_down(qlow, 1, WAVE);
      if ((tid & (WAVE - 1)) == 0) seam[tid / WAVE] = qlow;
    }
    s0[tid] = gk; s1[tid] = th;
    if (A.heights) s2[tid] = zr;       // (s2 is free inside the loop) level l needs the row of the layer above it too
    __syncthreads();
    const double gkn = has_up ? s0[tid + 1] : 0.0, thn = has_up ? s1[tid + 1] : 0.0;
    const double btl = dTB_dB * dbdT;
    double ct = gk * (w1 * awT + d1 * adT) + btl * Tm1 * (E * th);        // level l as the upper end of layer l
    double ce = gk * (w1 * awE + d1 * adE);
    ct += gkn * (w0n * awT + d0n * adT) + btl * Tl * thn;                 // ... and as the lower end of layer l+1
    ce += gkn * (w0n * awE + d0n * adE);
    if constexpr (RAY) {               // ... and through the refractive index of level l (and of the ground, level 0)
      if ((tid & (WAVE - 1)) == WAVE - 1 && has_up) pnn = seam[tid / WAVE + 1];
      pn += has_up ? pnn : 0.0;
      ct += pn * nT;
      ce += pn * nE;
    }
    double rl = 0.0, ri = 0.0;         // two more rows of a cloudy call; a profile without cloud in it has all-zero rows
    if (cloudy) {
      rl = gk * cst[nthr] + gkn * cst[2 * nthr];
      ri = gk * cst[5 * nthr] + gkn * cst[6 * nthr];
      ct += gk * cst[3 * nthr] + gkn * cst[4 * nthr];       // the liquid term of dTB/dT at fixed e (ice has no T tangent)
    }
    if (vars_call) {                   // the rows in the caller's variables, each element still in its register
      if (A.heights) {                 // thickness follows Tv of its two ends: folded into the T and humidity rows
        const double zn = has_up ? s2[tid + 1] : 0.0;
        ct += zr * vst[0] + zn * vst[nthr];
        ce += zr * vst[2 * nthr] + zn * vst[3 * nthr];
      }
      if (A.humidity) { ct += ce * vst[5 * nthr]; ce *= vst[4 * nthr]; }
      if (A.cloud && cloudy) {         // density falls with T at fixed mixing ratio
        ct -= rl * vst[7 * nthr] + ri * vst[8 * nthr];
        rl *= vst[6 * nthr]; ri *= vst[6 * nthr];
      }
    }
    if (live) {
      o_e[tid] = ce;
      if (o_z) o_z[tid] = zr;
      if (cloud_call) { if (o_l) o_l[tid] = rl; if (o_i) o_i[tid] = ri; }
      o_t[tid] = ct;
    }
    if (tid == 0) A.tb[row] = fdiv(hvk, Lg);
  }
  if constexpr (RAY) {
    // a trapped ray (ducting) left its elevation NaN and marks the profile 3, as the forward kernel does
    // (flag 2 outranks it: a cloudy call's workgroups of other frequencies may lower valid to 2 at any time, and this
    // workgroup leaves a 2 it sees alone; a 3 written first is overwritten by their 2)
    if (j == 0 && tid == 0 && duct[prof] && A.valid[prof] == 1) A.valid[prof] = 3;
  }
}

// dynamic LDS of a launch of either kernel: three rows + the scan's 16 wave sums, seven cloud rows, nine rows of the change
// of variables, the ray kernel's 3 x 16 seam values
inline size_t jac_rte_lds_bytes(const JacRteArgs& a, int threads, bool ray) {
  const bool cloud_call = a.denliq || a.denice;
  const bool vars_call = a.humidity || a.cloud || a.heights;
  const size_t rows = (cloud_call ? 10 : 3) + (vars_call ? JAC_VARS_ROWS : 0);
  return sizeof(double) * (rows * (size_t)threads + 16 + (ray ? 48 : 0));
}

}  // namespace mwrt
