// mwrt_tl.hip -- the device K-matrix path: tangent-linear absorption (k_absorb_tl) and the adjoint RTE that consumes it
// (k_jac_rte).  Declarations and argument records: mwrt_tl.hip.h; entry points: mwrt_absorption_tl_batch_device,
// mwrt_tb_jacobian_batch_device, mwrt_tb_jacobian_batch_opt_device (cloud liquid / ice) and
// mwrt_tb_jacobian_batch_vars_device (retrieval variables) in mwrt.hip; the mathematics: DESIGN.md sections 4.5 - 4.5.3.
#include "mwrt_tl.hip.h"
#include "mwrt_absorption.hip.h"      // level_state, goff_gratch_e, clog_, CLOUD_KICE (and the arithmetic of mwrt_math.hip.h)
#include "mwrt_tl_dev.hip.h"          // dd, hui_w_dw, layer_value_tl, the workgroup scans (shared with mwrt_par.hip)

namespace mwrt {

namespace {

// ---------------------------------------------------------------------------------------------
// k_absorb_tl: one wave = 64 levels of one profile x TL_NFC frequencies.  The per-(level, line) quantities and their
// tangents (width, shift, strength, mixing, ...) are formed once per chunk; per frequency the line shape and its two
// tangents are direct sums over every line.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_absorb_tl(const AbsorbTlArgs A) {
  constexpr int NFC = TL_NFC;
  const int lane = threadIdx.x;
  const int64_t prof = blockIdx.x / A.nslab;
  const int lev = (int)(blockIdx.x - prof * A.nslab) * WAVE + lane;
  const bool live = lev < A.nlev;
  const int jbase = blockIdx.y * NFC;
  const int nfc = min(NFC, A.nf - jbase);
  const cmodel M = (cmodel)A.M;
  const cdoubles cfrq = (cdoubles)A.frq;
  const int64_t off = prof * A.nlev + (live ? lev : A.nlev - 1);
  const double pin = A.p[off], tin = A.t[off], rhin = A.rh[off];
  double fq[NFC];
#pragma unroll
  for (int j = 0; j < NFC; ++j) fq[j] = cfrq[jbase + min(j, nfc - 1)];

  // RTEquation.vapor + the clearsky_absorption preamble, as the forward kernels evaluate it
  const double e0 = goff_gratch_e(tin, rhin);
  const LevelState L = level_state(pin, tin, e0);
  const double inv_t = fdiv(1.0, L.t);
  const double rvap = (0.01 * 8.314510) / 18.01528;
  const dd t = {L.t, 1.0, 0.0};
  const dd rho = {L.rho, -L.rho * inv_t, fdiv(1.0, rvap * L.t)};      // e / (rvap T)
  const double P = L.p;                                                 // total pressure: independent of T and e

  bool nan = isnan(pin) || isnan(tin) || isnan(rhin), neg = false;
  // stores of one species' three arrays: lanes = consecutive levels of one row (coalesced)
  auto store = [&](const dd (&a)[NFC], double* v, double* dt, double* de) {
    if (!live) return;
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
      if (j < nfc) {
        const int64_t o = (prof * A.nf + jbase + j) * A.nlev + lev;
        v[o] = a[j].v; dt[o] = a[j].t; de[o] = a[j].e;
        nan = nan || isnan(a[j].v);
        neg = neg || a[j].v < 0.0;
      }
    }
  };

  // ---- H2O lines + continuum (H2OAbsModel.h2o_absorption [EXT]) ----
  {
    dd wsum[NFC];
    const dd rt = rho * t;
    const dd pvap = fdiv(1.0, M->h2o_pvap_div) * rt;
    const dd pda = {P - pvap.v, -pvap.t, -pvap.e};
    const dd den = M->h2o_den_coef * rho;
    const dd lnc = {flog(fdiv(M->h2o_reftcon, L.t)), -inv_t, 0.0};
    const dd con0 = (M->h2o_cf * pda * dexp(M->h2o_xcf * lnc) + M->h2o_cs * pvap * dexp(M->h2o_xcs * lnc)) * pvap;
    const double tiv = fdiv(M->h2o_reftline, L.t);
    const dd ti = {tiv, -tiv * inv_t, 0.0};
    const dd tiln = {flog(tiv), -inv_t, 0.0};
    const dd ti2 = dexp(2.5 * tiln);
    const bool shifted = M->h2o_shift_mode != 0;
    dd sum[NFC];
#pragma unroll
    for (int j = 0; j < NFC; ++j) sum[j] = {0.0, 0.0, 0.0};
    for (int k = 0; k < M->n_h2o; ++k) {
      const auto& R = M->h2or[k];
      const dd w0 = R.w0 * pda * dexp(R.x * tiln) + R.w0s * pvap * dexp(R.xs * tiln);
      dd c1 = {R.fl, 0.0, 0.0};
      if (shifted) {
        dd sf = R.sh * pda, ss = R.shs * pvap;
        if (R.aair != 0.0) sf = sf * (1.0 + (-R.aair) * tiln);
        if (R.aself != 0.0) ss = ss * (1.0 + (-R.aself) * tiln);
        if (R.xh != 0.0) sf = sf * dexp(R.xh * tiln);
        if (R.xhs != 0.0) ss = ss * dexp(R.xhs * tiln);
        c1 = c1 + (sf + ss);
      }
      const dd wsq = w0 * w0;
      const dd s = R.s1 * ti2 * dexp(R.b2 * (1.0 + (-1.0) * ti));    // S / fl^2: the f^2 is applied at the end
      const dd base = ddiv(w0, wsq + 562500.0);
      const dd sw = s * w0, sbase = s * base;
      // speed-dependent resonant term (ABH2O_SD): per-(level, line) parts of Xc = A / B, A = w0 - 1.5 w2 + i (d1 + 1.5 delta2),
      // B = w2 - i delta2, and their tangents (dA is frequency independent: d(d1) = -d(c1))
      const bool sdline = M->h2o_w2[k] > 0.0;
      double sdlim = -1.0;
      cplx iB = {0.0, 0.0}, dA_t = {0.0, 0.0}, dA_e = {0.0, 0.0}, dB_t = {0.0, 0.0}, dB_e = {0.0, 0.0};
      double xre = 0.0, xim0 = 0.0;
      if (sdline) {
        const dd w2 = M->h2o_w2[k] * pda * dexp(M->h2o_xw2[k] * tiln) + M->h2o_w2s[k] * pvap * dexp(M->h2o_xw2s[k] * tiln);
        const dd d2 = M->h2o_d2[k] * pda + M->h2o_d2s[k] * pvap;
        iB = crecip(cplx{w2.v, -d2.v});
        sdlim = (w2.v > 0.0) ? 10.0 * w0.v : -1.0;
        xre = w0.v - 1.5 * w2.v; xim0 = 1.5 * d2.v;
        dA_t = {w0.t - 1.5 * w2.t, 1.5 * d2.t - c1.t}; dA_e = {w0.e - 1.5 * w2.e, 1.5 * d2.e - c1.e};
        dB_t = {w2.t, -d2.t}; dB_e = {w2.e, -d2.e};
      }
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = fq[j];
        const double d1 = f - c1.v, d2 = f + c1.v;
        const double D1 = __builtin_fma(d1, d1, wsq.v), D2 = __builtin_fma(d2, d2, wsq.v);
        const double D1t = __builtin_fma(-2.0 * d1, c1.t, wsq.t), D1e = __builtin_fma(-2.0 * d1, c1.e, wsq.e);
        const double D2t = __builtin_fma(2.0 * d2, c1.t, wsq.t), D2e = __builtin_fma(2.0 * d2, c1.e, wsq.e);
        const bool sd_in = fabs(d1) < sdlim;
        const double m1 = (fabs(d1) < 750.0 && !sd_in) ? 1.0 : 0.0;    // 750-GHz cutoff; the SD shape replaces term 1
        const double m2 = (fabs(d2) < 750.0) ? 1.0 : 0.0;
        const double num = __builtin_fma(m1, D2, m2 * D1);
        const double numt = __builtin_fma(m1, D2t, m2 * D1t), nume = __builtin_fma(m1, D2e, m2 * D1e);
        const double den12 = D1 * D2;
        const double dent = __builtin_fma(D1t, D2, D1 * D2t), dene = __builtin_fma(D1e, D2, D1 * D2e);
        const double r = fdiv(1.0, den12);
        const double q = num * r, qt = (numt - q * dent) * r, qe = (nume - q * dene) * r;
        const double mm = m1 + m2;
        sum[j].v = __builtin_fma(sw.v, q, __builtin_fma(-mm, sbase.v, sum[j].v));
        sum[j].t = __builtin_fma(sw.t, q, __builtin_fma(sw.v, qt, __builtin_fma(-mm, sbase.t, sum[j].t)));
        sum[j].e = __builtin_fma(sw.e, q, __builtin_fma(sw.v, qe, __builtin_fma(-mm, sbase.e, sum[j].e)));
        if (sdline && wave_any(sd_in)) {
          // Re SD and its tangents: with xrt = sqrt(Xc), pxw = sqrt(pi) xrt w(i xrt), SD = 2 (1 - pxw) / B,
          //   dSD = CA dA + CB dB,  CA = -2 K h / B^2,  CB = -CA Xc - SD / B,  K = sqrt(pi) (w + xrt w'),  h = 1 / (2 xrt)
          const cplx xc = cmul(cplx{xre, d1 + xim0}, iB);
          const cplx xrt = csqrt_principal(xc);
          cplx w, dw;
          hui_w_dw(xrt, w, dw);
          const double SQPI = 1.77245385090551603;
          const cplx pxw = cmul(cscale(xrt, SQPI), w);
          const cplx sdc = cmul(cplx{2.0 - 2.0 * pxw.re, -2.0 * pxw.im}, iB);
          const cplx K = cscale(caddc(w, cmul(xrt, dw)), SQPI);
          const cplx h = crecip(cscale(xrt, 2.0));
          const cplx CA = cscale(cmul(cmul(K, h), cmul(iB, iB)), -2.0);
          const cplx CB = csub(cplx{0.0, 0.0}, caddc(cmul(CA, xc), cmul(sdc, iB)));
          const double sdt = re_mul(CA, dA_t) + re_mul(CB, dB_t), sde = re_mul(CA, dA_e) + re_mul(CB, dB_e);
          const double r1 = sd_in ? sdc.re - base.v : 0.0;
          const double r1t = sd_in ? sdt - base.t : 0.0, r1e = sd_in ? sde - base.e : 0.0;
          sum[j].v = __builtin_fma(s.v, r1, sum[j].v);
          sum[j].t = __builtin_fma(s.t, r1, __builtin_fma(s.v, r1t, sum[j].t));
          sum[j].e = __builtin_fma(s.e, r1, __builtin_fma(s.v, r1e, sum[j].e));
        }
      }
    }
    const bool dry = !(L.rho > 0.0);
    const dd cden = 3.183e-05 * den;
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
      const double f2 = fq[j] * fq[j];
      dd a = f2 * (cden * sum[j] + con0);
      if (dry) a.v = 0.0;          // the value is zeroed at rho <= 0; the tangent is the right-sided one (continuous there)
      wsum[j] = a;
    }
    store(wsum, A.awet, A.dawet_dt, A.dawet_de);
  }

  // ---- O2 lines + non-resonant term + N2 continuum (O2AbsModel.o2_absorption / N2AbsModel [EXT]) ----
  {
    dd dsum[NFC];
    const double thv = fdiv(300.0, L.t);
    const dd th = {thv, -thv * inv_t, 0.0};
    const dd th1 = th + (-1.0);
    const dd lnth = {flog(thv), -inv_t, 0.0};
    const dd b = dexp(M->o2_x * lnth);
    const dd preswv = fdiv(1.0, M->o2_pvap_div) * (rho * t);
    const dd presda = {P - preswv.v, -preswv.t, -preswv.e};
    const dd den = 0.001 * (presda * b + M->o2_wv_factor * preswv * th);
    const dd dens = 0.001 * ((presda + M->o2_wv_factor * preswv) * th);
    const dd dfnr = M->o2_wb300 * den;
    const dd pe2 = den * den;
    const bool second = M->o2_mix_mode != 0;
    const dd ymul = second ? den : (0.001 * P) * b;
    const bool line1_dens = !second && M->o2_line1_dens;
    dd sum[NFC];
#pragma unroll
    for (int j = 0; j < NFC; ++j) sum[j] = {0.0, 0.0, 0.0};
    for (int k = 0; k < M->n_o2; ++k) {
      const auto& R = M->o2r[k];
      const dd y = ymul * (R.y1 * th1 + R.y0);
      dd dnu = {0.0, 0.0, 0.0}, gfac = {1.0, 0.0, 0.0};
      if (second) {
        dnu = pe2 * (R.dnu1 * th1 + R.dnu0);
        gfac = 1.0 + pe2 * (R.g1 * th1 + R.g0);
      }
      const dd df = R.w300 * ((k == 0 && line1_dens) ? dens : den);
      const dd str = R.s300rf2 * dexp(-R.be * th1);                   // S300 / F^2: the f^2 is applied at the end
      // n1 / D1 + n2 / D2 = (f^2 Pp + Qq) / (D1 D2),  Pp = 2 (a + c b), Qq = 2 (c^2 + w^2)(a - c b)  (the 2 is in scale2)
      const dd c1 = dnu + R.f;
      const dd df2 = df * df;
      const dd a = str * df * gfac;
      const dd cb = c1 * (str * y);
      const dd cc = c1 * c1 + df2;
      const dd Pp = a + cb, Qq = cc * (a - cb);
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = fq[j], f2 = f * f;
        const double d1 = f - c1.v, d2 = f + c1.v;
        const double D1 = __builtin_fma(d1, d1, df2.v), D2 = __builtin_fma(d2, d2, df2.v);
        const double D1t = __builtin_fma(-2.0 * d1, c1.t, df2.t), D1e = __builtin_fma(-2.0 * d1, c1.e, df2.e);
        const double D2t = __builtin_fma(2.0 * d2, c1.t, df2.t), D2e = __builtin_fma(2.0 * d2, c1.e, df2.e);
        const double den12 = D1 * D2;
        const double dent = __builtin_fma(D1t, D2, D1 * D2t), dene = __builtin_fma(D1e, D2, D1 * D2e);
        const double r = fdiv(1.0, den12);
        const double q = __builtin_fma(f2, Pp.v, Qq.v) * r;
        sum[j].v += q;
        sum[j].t = __builtin_fma(__builtin_fma(f2, Pp.t, Qq.t) - q * dent, r, sum[j].t);
        sum[j].e = __builtin_fma(__builtin_fma(f2, Pp.e, Qq.e) - q * dene, r, sum[j].e);
      }
    }
    const dd scale2 = (2.0 * M->o2_coef) * (presda * (th * th * th));
    const dd pn2 = M->n2_ptot ? dd{P, 0.0, 0.0} : dd{L.pdry, 0.0, -1.0};
    const dd n2c = (M->n2_n * M->n2_l) * (pn2 * pn2 * dexp(M->n2_m * lnth));
    const dd nr0 = (0.5 * M->o2_nonres) * dfnr;
    const dd dfnr2 = dfnr * dfnr;
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
      const double f = fq[j], f2 = f * f;
      double fdep = 1.0;
      if (M->n2_fdep) { const double qq = f * (1.0 / 450.0); fdep = 0.5 + fdiv(0.5, 1.0 + qq * qq); }
      const dd hnonres = ddiv(f2 * nr0, th * (dfnr2 + f2));
      dd o2 = scale2 * (f2 * sum[j] + hnonres);
      if (!(o2.v > 0.0)) o2 = {0.0, 0.0, 0.0};                       // max(o2abs, 0): no slope where it clamps
      dsum[j] = o2 + (fdep * f2) * n2c;
    }
    store(dsum, A.adry, A.dadry_dt, A.dadry_de);
  }

  if (A.flags) {
    const unsigned fl = (wave_any(live && nan) ? 1u : 0u) | (wave_any(live && neg) ? 2u : 0u);
    if (fl && lane == 0) atomicOr(A.flags + prof, fl);
  }
}

// ---------------------------------------------------------------------------------------------
// k_jac_rte: one workgroup per (profile, frequency), one lane per level.  Per frequency the layer values, their partial
// derivatives, the Planck terms and the zenith optical-depth prefix are formed once; per elevation the transmittances,
// one workgroup prefix sum (S_l = sum_{m <= l} c_m T_{m-1}) and a neighbour exchange give every level's three
// derivatives, which the lanes store as one contiguous row (level fastest: coalesced).
// ---------------------------------------------------------------------------------------------

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

__global__ void __launch_bounds__(1024)
k_jac_rte(const JacRteArgs A) {
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
  double tauz = lay ? Lw * dz + Ld * dz : 0.0;                         // zenith optical depth of layer l
  __syncthreads();
  s0[tid] = w0; s1[tid] = d0;          // the lower-end partials of layer l, for level l-1
  __syncthreads();
  const double w0n = has_up ? s0[tid + 1] : 0.0, d0n = has_up ? s1[tid + 1] : 0.0;
  if (cloudy) tauz = (tauz + tci) + tli;                              // the forward's order: ((wet + dry) + ice) + liquid
  double tau_tot;
  const double cum_in = block_scan(tauz, wsum, tid, nwaves, tau_tot);
  const double cum_ex = cum_in - tauz;                                   // zenith optical depth below layer l
  const double bbg = fdiv(1.0, fexp(fdiv(hvk, M->t_cosmic)) - 1.0);

  for (int a = 0; a < nang; ++a) {
    const double am = A.airmass[a];
    const int64_t row = (prof * nang + a) * nf + j;
    double* o_t = A.dtb_dt + row * nlev;
    double* o_e = A.dtb_de + row * nlev;
    double* o_z = A.dtb_ddz ? A.dtb_ddz + row * nlev : nullptr;
    double* o_l = A.dtb_dliq ? A.dtb_dliq + row * nlev : nullptr;
    double* o_i = A.dtb_dice ? A.dtb_dice + row * nlev : nullptr;
    if (isnan(am)) {                   // a NaN elevation: its rows are NaN, the profile stays valid
      if (live) { o_t[tid] = qnan; o_e[tid] = qnan; if (o_z) o_z[tid] = qnan; if (o_l) o_l[tid] = qnan; if (o_i) o_i[tid] = qnan; }
      if (tid == 0) A.tb[row] = qnan;
      continue;
    }
    const double tau = am * tauz;
    const double E = fexp(-tau);
    const double th = (tau <= EXP_SMALL_X) ? ftanh_half_small(tau) : fdiv(1.0 - E, 1.0 + E);   // (1 - E) / (1 + E)
    const double Tm1 = fexp(-am * cum_ex);                               // transmittance below layer l
    const double Tl = Tm1 * E;
    const double Pc = lay ? (bm + b * E) * th * Tm1 : 0.0;
    double Bsum;
    (void)block_scan(Pc, wsum, tid, nwaves, Bsum);
    const double Ttop = fexp(-am * tau_tot);
    const double Btot = (Ttop > TRANS_MIN) ? __builtin_fma(bbg, Ttop, Bsum) : Bsum;
    // radiance reaching the antenna from above layer l (sum_{m > l} c_m T_{m-1} + the cosmic term), summed directly:
    // B_tot - S_l would cancel to ~eps B_tot where it is tiny
    const double above = block_suffix_excl(Pc, wsum, tid, nwaves) + ((Ttop > TRANS_MIN) ? bbg * Ttop : 0.0);
    const double Lg = flog(1.0 + fdiv(1.0, Btot));
    const double dTB_dB = fdiv(hvk, Lg * Lg * Btot * (Btot + 1.0));
    const double opE = 1.0 + E;
    const double dc_dtau = fdiv(E * (2.0 * bm + 2.0 * b * E - b + b * E * E), opE * opE);
    const double g = lay ? dTB_dB * (Tm1 * dc_dtau - above) : 0.0;       // dTB / dtau_l (everything above l is dimmed)
    const double gk = g * am * dz;
    // dTB / d(thickness of layer l) [K/km]: tau_l = m (Lw + Ld + Ll + Li) dz_l is linear in dz_l, so this holds at
    // dz_l = 0 too
    const double zr = lay ? g * am * (cloudy ? (Lw + Ld) + cst[0] : Lw + Ld) : 0.0;
    s0[tid] = gk; s1[tid] = th;
    if (A.heights) s2[tid] = zr;       // (s2 is free inside the loop) level l needs the row of the layer above it too
    __syncthreads();
    const double gkn = has_up ? s0[tid + 1] : 0.0, thn = has_up ? s1[tid + 1] : 0.0;
    const double btl = dTB_dB * dbdT;
    double ct = gk * (w1 * awT + d1 * adT) + btl * Tm1 * (E * th);        // level l as the upper end of layer l
    double ce = gk * (w1 * awE + d1 * adE);
    ct += gkn * (w0n * awT + d0n * adT) + btl * Tl * thn;                 // ... and as the lower end of layer l+1
    ce += gkn * (w0n * awE + d0n * adE);
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
}

}  // namespace

hipError_t launch_absorb_tl(const AbsorbTlArgs& a, int64_t nprof, hipStream_t st) {
  const dim3 grid((unsigned)(nprof * a.nslab), (unsigned)((a.nf + TL_NFC - 1) / TL_NFC));
  hipLaunchKernelGGL(k_absorb_tl, grid, dim3(WAVE), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_jac_rte(const JacRteArgs& a, int64_t nprof, hipStream_t st) {
  const int threads = ((a.nlev + WAVE - 1) / WAVE) * WAVE;
  const bool cloud_call = a.denliq || a.denice;                    // seven more rows: the per-level cloud terms
  const bool vars_call = a.humidity || a.cloud || a.heights;       // nine more: the factors of the change of variables
  const size_t rows = (cloud_call ? 10 : 3) + (vars_call ? JAC_VARS_ROWS : 0);
  const size_t lds = sizeof(double) * (rows * (size_t)threads + 16);
  // beyond the default dynamic LDS limit: cloudy launches above 768 levels; with retrieval variables clear launches above
  // 640 levels (12 rows) and cloudy ones above 384 (19 rows: 152 KiB at 1024 levels, inside the 160 KiB of a workgroup)
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_jac_rte),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_jac_rte, dim3((unsigned)(nprof * a.nf)), dim3(threads), lds, st, a);
  return hipGetLastError();
}

}  // namespace mwrt
