// mwrt_tl.hip -- the device K-matrix path: tangent-linear absorption (k_absorb_tl) and the adjoint RTE that consumes it
// (k_jac_rte).  Declarations and argument records: mwrt_tl.hip.h; entry points: mwrt_absorption_tl_batch_device,
// mwrt_tb_jacobian_batch_device, mwrt_tb_jacobian_batch_opt_device (cloud liquid / ice) and
// mwrt_tb_jacobian_batch_vars_device (retrieval variables) in mwrt.hip; the mathematics: DESIGN.md sections 4.5 - 4.5.3.
#include "mwrt_tl.hip.h"
#include "mwrt_absorption.hip.h"      // level_state, goff_gratch_e, clog_, CLOUD_KICE (and the arithmetic of mwrt_math.hip.h)
#include "mwrt_tl_dev.hip.h"          // dd, hui_w_dw, layer_value_tl, the workgroup scans (shared with mwrt_par.hip)
#include "mwrt_tl_rte.hip.h"          // jac_rte_body: the adjoint RTE (shared with mwrt_ray.hip)

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
// derivatives, which the lanes store as one contiguous row (level fastest: coalesced).  The body is jac_rte_body
// (mwrt_tl_rte.hip.h), shared with the ray-traced kernel of mwrt_ray.hip; this is its plane-parallel form.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_jac_rte(const JacRteArgs A) {
  jac_rte_body<false>(A, nullptr, nullptr);
}

}  // namespace

hipError_t launch_absorb_tl(const AbsorbTlArgs& a, int64_t nprof, hipStream_t st) {
  const dim3 grid((unsigned)(nprof * a.nslab), (unsigned)((a.nf + TL_NFC - 1) / TL_NFC));
  hipLaunchKernelGGL(k_absorb_tl, grid, dim3(WAVE), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_jac_rte(const JacRteArgs& a, int64_t nprof, hipStream_t st) {
  const int threads = ((a.nlev + WAVE - 1) / WAVE) * WAVE;
  // three rows; seven more with cloud arrays (the per-level cloud terms), nine more with a retrieval-variable mode
  const size_t lds = jac_rte_lds_bytes(a, threads, false);
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
