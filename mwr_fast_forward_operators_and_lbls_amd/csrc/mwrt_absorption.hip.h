// mwrt_absorption.hip.h -- K1, absorption at one level (= one lane) for the frequencies of a chunk: the per-level
// state, the H2O and O2 line sums with their far-line forms, the continua, the opt-in species and cloud models and
// the refractive index.  Used by the fused kernel, the absorption kernels and (in parts) the K-matrix kernels.
#pragma once
#include "mwrt_math.hip.h"

namespace mwrt {

// The sets depend on the chunk's frequencies and the table only: the host computes them once per (model, frequency
// list, chunk width) -- csrc/mwrt_plan.cpp chunk_masks() -- and the kernels fetch their chunk's record through the scalar
// cache (round 2 had every workgroup derive them: ~180 VALU per lane and chunk).
typedef const __attribute__((address_space(4))) LineMasks* cmasks;
__device__ __forceinline__ LineMasks load_masks(const LineMasks* table, int chunk) {
  const cmasks q = (cmasks)table + chunk;
  LineMasks lm;
  lm.o2_far = q->o2_far; lm.h2o_far = q->h2o_far; lm.h2o_none = q->h2o_none; lm.h2o_res = q->h2o_res; lm.h2o_sd = q->h2o_sd;
  lm.h2o_sdfar = q->h2o_sdfar; lm.h2o_sdint = q->h2o_sdint;
  lm.h2o_vfar = q->h2o_vfar; lm.o2_vfar = q->o2_vfar; lm.vf_u0 = q->vf_u0; lm.vf_h = q->vf_h; lm.vf_invh = q->vf_invh;
  return lm;
}

// ---------------------------------------------------------------------------------------------
// per-level state shared by the H2O / O2 / N2 evaluations (RTEquation.vapor +
// clearsky_absorption preamble [EXT], incl. pyrtlib's kPa round trip)
// ---------------------------------------------------------------------------------------------
struct LevelState {
  double t;       // K    (300/(300/tk))
  double p;       // hPa  ((pdrykpa+ekpa)*10)
  double rho;     // g m-3
  double pdry;    // hPa  (pdrykpa*10)
};

__device__ __forceinline__ double goff_gratch_e(double tk, double rh) {
  const double LN10 = 2.302585092994045684;
  const double INV_LN10 = 0.434294481903251828;
  double y = 373.16 / tk;
  double es = -7.90298 * (y - 1.0) + 5.02808 * (flog(y) * INV_LN10)
            - 1.3816e-07 * (fexp(LN10 * (11.344 * (1.0 - (1.0 / y)))) - 1.0)
            + 0.0081328 * (fexp(LN10 * (-3.49149 * (y - 1.0))) - 1.0) + 3.0057148979490314 /*log10(1013.246)*/;
  return rh * fexp(LN10 * es);
}

__device__ __forceinline__ LevelState level_state(double p_hpa, double tk, double e) {
  const double rvap = (0.01 * 8.314510) / 18.01528;
  double v = 300.0 / tk;
  double ekpa = e / 10.0;
  double pdrykpa = p_hpa / 10.0 - ekpa;
  LevelState s;
  s.t = 300.0 / v;
  s.p = (pdrykpa + ekpa) * 10.0;
  s.rho = ekpa * 10.0 / (rvap * s.t);
  s.pdry = pdrykpa * 10.0;
  return s;
}

// ---------------------------------------------------------------------------------------------
// K1a: H2O lines + continuum for NFC uniform frequencies (H2OAbsModel.h2o_absorption [EXT])
//
// Per line the two Lorentz terms share ONE reciprocal:
//   s*[m1*(w/(D1) - base) + m2*(w/(D2) - base)] = (s w) (m1 D2 + m2 D1)/(D1 D2) - (m1+m2)(s base)
// with m = 1.0/0.0 for the 750-GHz cutoff.  The speed-dependent 22/183-GHz resonant term is
// evaluated in a second, short loop over the SD lines only (keeps the hot loop branch-free).
// ---------------------------------------------------------------------------------------------
struct H2OLine {          // per-(level, line) quantities, frequency independent
  double c1;              // line centre + pressure shift
  double w0, wsq;         // half width, squared
  double sw;              // S/fl^2 * w0
  double sbase;           // S/fl^2 * base
  double s;               // S/fl^2
  double base;
};

__device__ __forceinline__ H2OLine h2o_line(cmodel M, int k, double pda, double pvap, double ti, double tiln,
                                            double ti2, bool shifted) {
  H2OLine q;
  const auto& R = M->h2or[k];
  const double fl = R.fl;
  q.w0 = R.w0 * pda * fexp(R.x * tiln) + R.w0s * pvap * fexp(R.xs * tiln);
  double shift = 0.0;
  if (shifted) {
    // exponents / ln-T coefficients that are zero in the table cost nothing (uniform branches)
    const double xh = R.xh, xhs = R.xhs, aa = R.aair, as = R.aself;
    double sf = R.sh * pda, ss = R.shs * pvap;
    if (aa != 0.0) sf *= (1.0 - aa * tiln);
    if (as != 0.0) ss *= (1.0 - as * tiln);
    if (xh != 0.0) sf *= fexp(xh * tiln);
    if (xhs != 0.0) ss *= fexp(xhs * tiln);
    shift = sf + ss;
  }
  q.wsq = q.w0 * q.w0;
  q.s = R.s1 * ti2 * fexp(R.b2 * (1.0 - ti));                 // R.s1 = S1 / fl^2: the f^2 is applied at the end
  q.base = fdiv1(q.w0, 562500.0 + q.wsq);
  q.c1 = fl + shift;
  q.sw = q.s * q.w0;
  q.sbase = q.s * q.base;
  return q;
}

// Far-line bodies shared by the H2O and O2 loops: the two Lorentz terms of a line whose centre is
// far from every frequency of the chunk collapse to one rational function of f^2,
//   (f^2 P + Q) / (f^4 + A2 f^2 + Bc),   A2 = 2 (w^2 - c^2),  Bc = (c^2 + w^2)^2
// (cancellation in the denominator <= f^2 / (4 FAR_MIN^2) ulp ~ 2e-12).
struct FarLine { double P, Q, A2, Bc; };

// FOUR far lines per frequency through ONE reciprocal:
//   n0/d0 + n1/d1 + n2/d2 + n3/d3 = ((n0 d1 + n1 d0) d2 d3 + (n2 d3 + n3 d2) d0 d1) / (d0 d1 d2 d3).
// v_rcp_f64 costs about three FMA issue slots and delivers 2^-23, so a reciprocal + Newton step is 5 of
// the 9 slots a line-frequency term costs on its own; shared by four lines the term costs 6.6.
// 24 FMA-class instructions + 1 rcp per frequency (products stay < 1e48 for centres <= 1 THz).
// A wave issues in order, and a SIMD holds only three of these waves: the reciprocal and the Newton step that end a
// frequency are a serial tail, and the compiler (scheduling for register pressure) runs one frequency after the other.
// Here two frequencies go side by side and the loop is software-pipelined by hand: the reciprocals of one pair are issued,
// then the 52 independent instructions of the NEXT pair's numerators and denominators, then the first pair's Newton step and
// accumulation; the f^2 values are read from LDS two pairs ahead.  Scheduling barriers keep the compiler from undoing it.
// the quad at one frequency, num / den with den = d0 d1 d2 d3: 21 instructions
__device__ __forceinline__ void far_quad_terms(double f2, const FarLine& a, const FarLine& b, const FarLine& c, const FarLine& d,
                                               double& den, double& num) {
  const double d0 = __builtin_fma(f2, f2 + a.A2, a.Bc);
  const double d1 = __builtin_fma(f2, f2 + b.A2, b.Bc);
  const double d2 = __builtin_fma(f2, f2 + c.A2, c.Bc);
  const double d3 = __builtin_fma(f2, f2 + d.A2, d.Bc);
  const double n0 = __builtin_fma(f2, a.P, a.Q);
  const double n1 = __builtin_fma(f2, b.P, b.Q);
  const double n2 = __builtin_fma(f2, c.P, c.Q);
  const double n3 = __builtin_fma(f2, d.P, d.Q);
  const double p01 = d0 * d1, p23 = d2 * d3;
  const double m01 = __builtin_fma(n0, d1, n1 * d0);
  const double m23 = __builtin_fma(n2, d3, n3 * d2);
  den = p01 * p23;
  num = __builtin_fma(m01, p23, m23 * p01);
}
template <int NFC>
__device__ __forceinline__ void far_quad_accumulate(const double* sfq, const FarLine& a, const FarLine& b,
                                                    const FarLine& c, const FarLine& d, double (&sum)[NFC]) {
  static_assert(NFC % 2 == 0, "frequencies are taken in pairs");
  auto front = [&](const double (&f2s)[2], double (&den)[2], double (&num)[2]) {
#pragma unroll
    for (int g = 0; g < 2; ++g) far_quad_terms(f2s[g], a, b, c, d, den[g], num[g]);
  };
  double den[2], num[2], r[2];
  double f2c[2] = {sfq[1], sfq[3]};
  double f2n[2] = {sfq[(NFC > 2) ? 5 : 1], sfq[(NFC > 2) ? 7 : 3]};
  front(f2c, den, num);
  r[0] = __builtin_amdgcn_rcp(den[0]); r[1] = __builtin_amdgcn_rcp(den[1]);
#pragma unroll
  for (int j = 0; j < NFC; j += 2) {
    double den_n[2] = {1.0, 1.0}, num_n[2] = {0.0, 0.0}, f2p[2] = {0.0, 0.0};
    if (j + 4 < NFC) { f2p[0] = sfq[2 * (j + 4) + 1]; f2p[1] = sfq[2 * (j + 5) + 1]; }      // in flight for two trips
    MWRT_STAGE();
    if (j + 2 < NFC) front(f2n, den_n, num_n);
    MWRT_STAGE();
    const double e0 = __builtin_fma(-den[0], r[0], 1.0), e1 = __builtin_fma(-den[1], r[1], 1.0);
    r[0] = __builtin_fma(r[0], e0, r[0]); r[1] = __builtin_fma(r[1], e1, r[1]);
    sum[j] = __builtin_fma(num[0], r[0], sum[j]); sum[j + 1] = __builtin_fma(num[1], r[1], sum[j + 1]);
    if (j + 2 < NFC) {
      den[0] = den_n[0]; den[1] = den_n[1]; num[0] = num_n[0]; num[1] = num_n[1];
      r[0] = __builtin_amdgcn_rcp(den[0]); r[1] = __builtin_amdgcn_rcp(den[1]);
      f2n[0] = f2p[0]; f2n[1] = f2p[1];
    }
  }
  MWRT_STAGE();
}

// SEVERAL quads per reciprocal (the fused kernel): the far-line sum of a frequency is carried across the quads of a group
// as a fraction N / D and divided out once per group.  With S the plain sum so far,
//   first quad of a group   N = S den + num,           D = den              (1 instruction behind the 21 of the quad)
//   each later quad         N = N den + num D,         D = D den            (3)
//   end of the group        S = N (1 / D)                                   (v_rcp_f64 + Newton step + multiply, as before)
// so nine quads in groups of 5 + 4 end in two reciprocals per frequency instead of nine.  Nothing in a quad waits for a
// reciprocal any more: the frequencies are independent chains of FMAs and the compiler interleaves them as it likes; the
// reciprocals of a group's end go side by side for all frequencies.  A line voted out at set-up (P = Q = 0) stays in its
// quad: its denominator multiplies D, its numerator is zero.
// Range of D: a far line has |f - c| >= FAR_MIN_GHZ = 0.2 GHz after its shift, so with centres and frequencies in
// [1 GHz, 1 THz] and half widths up to 5 GHz a line's denominator ((f - c)^2 + w^2)((f + c)^2 + w^2) lies in
// [0.04, 1.01e12] and a quad's in [2.5e-6, 1.05e48]: a group of FAR_GROUP_QUADS = 5 reaches D in [1e-28, 1e241], a factor
// 1e67 under the overflow threshold (1.8e308) and 1e279 above the smallest normal number.  N is at most sum|term| D, and
// the sums (S / F^2-scaled line strengths over such denominators) are far below 1e17, which leaves the 1e50 of headroom
// this form is held to (tests/test_far_group_reference.py).  The 1 THz is the API's stated frequency limit (include/mwrt.h,
// "Frequencies"); the headroom holds to about 1.6 THz (D grows as f^80), and from about 7 THz a group's product overflows.  Six quads (1.3e288) would still fit, without the headroom;
// nine (1e432) overflow.
constexpr int FAR_GROUP_QUADS = 5;
// A later quad updates N where it lives.  The compiler forms the product num D first and lets a v_fmac accumulate into it:
// the new N then sits beside the old one, and NFC 64-bit copies carry it back at the loop's latch.  The three-address form
// of the same FMA, destination = first factor, is written out here instead (same operands, same operation, same bits).
__device__ __forceinline__ void fma_in_place(double& n, double den, double t) {          // n = fma(n, den, t)
  asm("v_fma_f64 %0, %0, %1, %2" : "+v"(n) : "v"(den), "v"(t));
}
template <int NFC, bool FIRST>
__device__ __forceinline__ void far_quad_fraction(const double* sfq, const FarLine& a, const FarLine& b, const FarLine& c,
                                                  const FarLine& d, const double (&sum)[NFC], double (&N)[NFC], double (&D)[NFC]) {
#pragma unroll
  for (int j = 0; j < NFC; ++j) {
    double den, num;
    far_quad_terms(sfq[2 * j + 1], a, b, c, d, den, num);
    if constexpr (FIRST) {
      N[j] = __builtin_fma(sum[j], den, num);
      D[j] = den;
    } else {
      fma_in_place(N[j], den, num * D[j]);
      D[j] *= den;
    }
  }
}
template <int NFC>
__device__ __forceinline__ void far_group_close(const double (&N)[NFC], const double (&D)[NFC], double (&sum)[NFC]) {
  double r[NFC];
#pragma unroll
  for (int j = 0; j < NFC; ++j) r[j] = __builtin_amdgcn_rcp(D[j]);
#pragma unroll
  for (int j = 0; j < NFC; ++j) r[j] = __builtin_fma(r[j], __builtin_fma(-D[j], r[j], 1.0), r[j]);
#pragma unroll
  for (int j = 0; j < NFC; ++j) sum[j] = N[j] * r[j];
}
// the quad loop of a species in this form: `m` holds a multiple of four lines, `setup(k, FarLine&)` is the species' far_setup
template <int NFC, class Mask, class Setup>
__device__ __forceinline__ void far_groups_accumulate(const double* sfq, Mask m, Setup&& setup, double (&sum)[NFC]) {
  auto next_quad = [&](FarLine (&q)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { setup(__builtin_ctzll((unsigned long long)m), q[i]); m &= m - Mask(1); }
    LDS_RELOAD_FENCE();
  };
  while (m) {
    double N[NFC], D[NFC];
    {
      FarLine q[4];
      next_quad(q);
      far_quad_fraction<NFC, true>(sfq, q[0], q[1], q[2], q[3], sum, N, D);
    }
    for (int g = 1; g < FAR_GROUP_QUADS && m; ++g) {
      FarLine q[4];
      next_quad(q);
      far_quad_fraction<NFC, false>(sfq, q[0], q[1], q[2], q[3], sum, N, D);
    }
    far_group_close<NFC>(N, D, sum);
  }
}

// VERY far lines: a line whose poles in u = f^2 (u ~ c^2 -+ 2 i c w) lie at >= 1/VF_RATIO_MAX half ranges from the middle u0
// of the chunk's f^2 values -- the submillimetre lines seen from a 22-58 GHz chunk -- is analytic across the chunk with
// room to spare: its term (P u + Q)/(u^2 + A2 u + Bc) is expanded in x = (u - u0)/h, |x| <= 1,
//   d(u) = d0 + d1 h x + h^2 x^2,   c_0 = n(u0)/d0,  c_1 = (P h - d1 h c_0)/d0,  c_j = -(d1 h c_{j-1} + h^2 c_{j-2})/d0,
// and ALL such lines of a species share one polynomial: ~40 instructions per line instead of 7 per line and frequency, plus
// one Horner evaluation per frequency.  Truncation after x^7: sum_{j>=8} (j+1) r^j <= 4e-14 of the line's own term at
// r = VF_RATIO_MAX (the poles' distance ratio), and such a line is a few percent of the absorption at most; the host picks
// the lines (chunk_masks) with the shift / width allowances.
constexpr int VF_TERMS = 8;                  // (VF_RATIO_MAX, VF_MIN_FREQS, VF_MIN_LINES: mwrt_plan.h)
__device__ __forceinline__ void vfar_add(const FarLine& fl, double u0, double h, double (&acc)[VF_TERMS]) {
  const double d0 = __builtin_fma(u0, u0 + fl.A2, fl.Bc);
  const double d1h = __builtin_fma(fl.A2, h, (2.0 * u0) * h);
  double rd = __builtin_amdgcn_rcp(d0);
  rd = __builtin_fma(rd, __builtin_fma(-d0, rd, 1.0), rd);
  const double a = -d1h * rd, b = (-(h * h)) * rd;
  double cm2 = __builtin_fma(fl.P, u0, fl.Q) * rd;
  double cm1 = __builtin_fma(a, cm2, (fl.P * h) * rd);
  acc[0] += cm2;
  acc[1] += cm1;
#pragma unroll
  for (int j = 2; j < VF_TERMS; ++j) {
    const double cj = __builtin_fma(a, cm1, b * cm2);
    acc[j] += cj;
    cm2 = cm1; cm1 = cj;
  }
}
template <int NFC>
__device__ __forceinline__ void vfar_eval(const double* sfq, double invh, double mu /* = -u0 / h */, const double (&acc)[VF_TERMS], double (&sum)[NFC]) {
  // the Horner chains of several frequencies side by side (each is VF_TERMS - 1 dependent FMAs)
  constexpr int G = (NFC % 7 == 0) ? 7 : ((NFC % 4 == 0) ? 4 : 2);
  static_assert(NFC % G == 0, "group width");
#pragma unroll
  for (int j0 = 0; j0 < NFC; j0 += G) {
    double x[G], p[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { x[g] = __builtin_fma(sfq[2 * (j0 + g) + 1], invh, mu); p[g] = acc[VF_TERMS - 1]; }
#pragma unroll
    for (int k = VF_TERMS - 2; k >= 0; --k) {
#pragma unroll
      for (int g = 0; g < G; ++g) p[g] = __builtin_fma(p[g], x[g], acc[k]);
      MWRT_STAGE();
    }
#pragma unroll
    for (int g = 0; g < G; ++g) sum[j0 + g] += p[g];
  }
}

// ... and TWO far lines through one reciprocal (what a quad loop leaves over, when it leaves two or three)
template <int NFC>
__device__ __forceinline__ void far_pair_accumulate(const double* sfq, const FarLine& a, const FarLine& b, double (&sum)[NFC]) {
#pragma unroll
  for (int j = 0; j < NFC; ++j) {
    const double f2 = sfq[2 * j + 1];
    const double d0 = __builtin_fma(f2, f2 + a.A2, a.Bc);
    const double d1 = __builtin_fma(f2, f2 + b.A2, b.Bc);
    const double n0 = __builtin_fma(f2, a.P, a.Q);
    const double n1 = __builtin_fma(f2, b.P, b.Q);
    const double den = d0 * d1;
    const double num = __builtin_fma(n0, d1, n1 * d0);
    double r = __builtin_amdgcn_rcp(den);
    r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
    sum[j] = __builtin_fma(num, r, sum[j]);
  }
}

// lowest `n` set bits of `m` (n < 4): the lines a quad loop leaves to the general loop
__device__ __forceinline__ unsigned long long lowest_bits(unsigned long long m, int n) {
  unsigned long long out = 0;
  for (int i = 0; i < n; ++i) { const unsigned long long b = m & (0ull - m); out |= b; m ^= b; }
  return out;
}

// Half-sampled speed-dependent shape (16-frequency chunks of a fine grid, chunk >= 3 GHz and 5 spans from the line centre).
// The SD resonant shape costs ~92 VALU per (level, frequency); its DIFFERENCE from the Lorentzian it replaces is small
// (<= 2 % of it) and smooth across a chunk, so it is evaluated at 9 of the 16 frequencies (slots 0, 2, ..., 14 and 15) and
// interpolated to the other 7 with host-computed Lagrange weights: error <= 4e-12 of the line's Lorentzian
// (probe on the oracle's formulas; 1.8e-12 of the wet absorption at exactly 5 spans, tests/window_reference.py),
// against the 3e-10 the window plan itself leaves.  The host half-samples only chunks whose own slots interpolate stably
// (SD_LEBESGUE_MAX, mwrt_plan.h).  Where a lane is inside 10
// half-widths the odd slots then get Lorentzian + interpolated difference; outside, the plain Lorentzian as always.
// (SD_NODES, SD_TARGETS, sd_node_slot: mwrt_plan.h)

// Window mode (k_absorb_win, fine spectral grids).  The lines far from a whole WINDOW of chunks are summed at a few
// Chebyshev nodes of the window (NODES = true: raw line sums out, no continuum, no SD lines; a line whose per-lane
// vote fails is reported in *failed and left out) and interpolated to each chunk's frequencies; the chunk call then
// starts from those sums (init_sum, init_bsum) and skips the lines in `excl`.  Outside window mode: excl = 0, null.
// GROUPED: the far quads as running fractions (far_groups_accumulate) -- the fused kernel up to 512 threads, all variants alike
template <int NFC, bool NODES = false, bool GROUPED = false>
__device__ __forceinline__ void h2o_absorb(cmodel M, const LevelState& L, const double* sfq /*LDS: {f, f^2} per slot*/,
                                           const LineMasks& lm, double (&awet)[NFC], unsigned excl = 0u,
                                           const double* init_sum = nullptr, double init_bsum = 0.0,
                                           unsigned* failed = nullptr, double* bsum_out = nullptr,
                                           cdoubles sdw = nullptr /* [SD_TARGETS][SD_NODES] weights of this chunk, or null */) {
  const double t = L.t;
  const double pvap = fdiv(L.rho * t, M->h2o_pvap_div);
  const double pda = L.p - pvap;
  const double den = M->h2o_den_coef * L.rho;
  const double lnc = flog(fdiv(M->h2o_reftcon, t));
  const double con0 = (M->h2o_cf * pda * fexp(M->h2o_xcf * lnc) + M->h2o_cs * pvap * fexp(M->h2o_xcs * lnc)) * pvap;
  const double ti = fdiv(M->h2o_reftline, t);
  const double tiln = flog(ti);
  const double ti2 = fexp(2.5 * tiln);
  const bool shifted = M->h2o_shift_mode != 0;
  double sum[NFC];
#pragma unroll
  for (int j = 0; j < NFC; ++j) sum[j] = init_sum ? init_sum[j] : 0.0;

  const int nl = M->n_h2o;
  const unsigned all = h2o_lines_all(nl) & ~excl;
  // The 750-GHz cutoff of each Lorentz term depends on the lane only through the (tiny) pressure
  // shift.  Three loops, each with ONE body:
  //   A  far lines (table centre >= FAR_H2O_GHZ from every frequency), both terms inside the cutoff for
  //      every lane (wave vote at the chunk's extreme frequencies): the rational form, no masks.
  //      A line that fails the vote is handed to loop B.
  //   B  everything else that is not speed dependent: resonant-only / near-centre / masked forms.
  //   C  speed-dependent lines (22 / 183 GHz in R20SD+): Lorentz pair + the SD resonant shape.
  // Lines whose two terms are beyond the cutoff for every frequency (e.g. 916 GHz from 22 GHz) are skipped.
  const double fmin = sfq[2 * NFC], fmax = sfq[2 * NFC + 1];
  double bsum = init_bsum;                                    // sum of (count * s * base), frequency independent
  const unsigned sd_eff = h2o_sd_near(lm);                    // lines that go to the speed-dependent loop straight away
  unsigned sd_extra = 0u;                                     // ... and the "out of reach" ones a level of this wave takes back
  unsigned deferred = (~lm.h2o_far | lm.h2o_res) & ~sd_eff & ~lm.h2o_none & all;
  const unsigned setA = (MWRT_ABLATE & 2) ? 0u : h2o_far_set(lm, all);
  // ... of which the very far ones go through one Taylor polynomial (vfar_add) and the rest
  // FOUR at a time through far_quad_accumulate; the count mod 4 left over joins loop B
  const unsigned setV = h2o_vfar_set(lm, setA, NODES);
  const unsigned setQ = h2o_quad_set(lm, setA, NODES);
  const unsigned leftA = (unsigned)lowest_bits(setQ, __builtin_popcount(setQ) & 3);
  const unsigned leftP = (__builtin_popcount(leftA) >= 2) ? (unsigned)lowest_bits(leftA, 2) : 0u;      // ... two of them as a pair
  deferred |= leftA & ~leftP;
  auto far_setup = [&](int k, FarLine& fl) {
    const H2OLine q = h2o_line(M, k, pda, pvap, ti, tiln, ti2, shifted);
    // both terms inside the cutoff for every lane?
    const bool plain = wave_all_of(q.c1 - fmin < 750.0, fmax - q.c1 < 750.0, q.c1 - fmin > -750.0, fmax + q.c1 < 750.0, fmin + q.c1 > -750.0);
    // both terms in:  s w (D1 + D2)/(D1 D2) - 2 s base,  D1 + D2 = 2 f^2 + 2 (c^2 + w^2)
    const double cc = __builtin_fma(q.c1, q.c1, q.wsq);
    fl.A2 = 2.0 * __builtin_fma(-q.c1, q.c1, q.wsq);
    fl.Bc = cc * cc;
    double P = 2.0 * q.sw, bs = 2.0 * q.sbase;
    // a speed-dependent line is a plain line only where its special shape (inside 10 half-widths, ABH2O_SD) is out of
    // reach of every frequency in [fmin, fmax] at this level
    const bool sdline = M->h2o_w2[k] > 0.0;
    const bool reach = sdline && !wave_all(10.0 * q.w0 < ::fmin(fabs(q.c1 - fmin), fabs(q.c1 - fmax)));
    if (reach || !plain) {                                                // SD within reach / cutoff not uniform
      if constexpr (NODES) *failed |= 1u << k;
      else if (reach) sd_extra |= 1u << k;                                       // ... the speed-dependent loop's job
      else deferred |= 1u << k;                                                  // ... loop B's job
      P = 0.0; bs = 0.0;
    }
    fl.P = P;
    fl.Q = P * cc;
    bsum += bs;
  };
  if (setV) {
    double acc[VF_TERMS];
#pragma unroll
    for (int j = 0; j < VF_TERMS; ++j) acc[j] = 0.0;
    for (unsigned m = setV; m; m &= m - 1u) {
      FarLine q;
      far_setup(__builtin_ctz(m), q);
      vfar_add(q, lm.vf_u0, lm.vf_h, acc);
    }
    LDS_RELOAD_FENCE();
    vfar_eval<NFC>(sfq, lm.vf_invh, -lm.vf_u0 * lm.vf_invh, acc, sum);
  }
  if constexpr (GROUPED) far_groups_accumulate<NFC>(sfq, setQ & ~leftA, far_setup, sum);
  else for (unsigned m = setQ & ~leftA; m;) {
    FarLine q0, q1, q2, q3;
    far_setup(__builtin_ctz(m), q0); m &= m - 1u;
    far_setup(__builtin_ctz(m), q1); m &= m - 1u;
    far_setup(__builtin_ctz(m), q2); m &= m - 1u;
    far_setup(__builtin_ctz(m), q3); m &= m - 1u;
    LDS_RELOAD_FENCE();
    far_quad_accumulate<NFC>(sfq, q0, q1, q2, q3, sum);
  }
  if (leftP) {
    FarLine q0, q1;
    unsigned m = leftP;
    far_setup(__builtin_ctz(m), q0); m &= m - 1u;
    far_setup(__builtin_ctz(m), q1);
    LDS_RELOAD_FENCE();
    far_pair_accumulate<NFC>(sfq, q0, q1, sum);
  }
  if (MWRT_ABLATE & 2) deferred = 0u;
  for (unsigned m = deferred; m; m &= m - 1u) {
    const int k = __builtin_ctz(m);
    const H2OLine q = h2o_line(M, k, pda, pvap, ti, tiln, ti2, shifted);
    const bool d1_in = (q.c1 - fmin < 750.0) && (fmax - q.c1 < 750.0) && (q.c1 - fmin > -750.0);
    const bool d1_out = (q.c1 - fmax >= 750.0) || (fmin - q.c1 >= 750.0);
    const bool d2_in = fmax + q.c1 < 750.0 && fmin + q.c1 > -750.0;
    const bool d2_out = fmin + q.c1 >= 750.0;
    if (wave_all(d1_out && d2_out)) continue;
    if (M->h2o_w2[k] > 0.0 && !wave_all(10.0 * q.w0 < ::fmin(fabs(q.c1 - fmin), fabs(q.c1 - fmax)))) {
      // a speed-dependent line within reach of its special shape: not a plain line at this level
      if constexpr (NODES) *failed |= 1u << k; else sd_extra |= 1u << k;
      continue;
    }
    LDS_RELOAD_FENCE();
    if (wave_all(d1_in && d2_in)) {                               // next to a line centre: detunings formed directly
      bsum = __builtin_fma(2.0, q.sbase, bsum);
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = sfq[2 * j];
        const double d1 = f - q.c1;
        const double d2 = f + q.c1;
        const double D1 = __builtin_fma(d1, d1, q.wsq);
        const double D2 = __builtin_fma(d2, d2, q.wsq);
        const double den12 = D1 * D2;
        double r = __builtin_amdgcn_rcp(den12);
        r = __builtin_fma(r, __builtin_fma(-den12, r, 1.0), r);
        sum[j] = __builtin_fma((D1 + D2) * r, q.sw, sum[j]);
      }
    } else if (wave_all(d1_in && d2_out)) {                       // resonant term only (e.g. 752 GHz seen from 22 GHz)
      bsum += q.sbase;
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double d1 = sfq[2 * j] - q.c1;
        const double D1 = __builtin_fma(d1, d1, q.wsq);
        double r = __builtin_amdgcn_rcp(D1);
        r = __builtin_fma(r, __builtin_fma(-D1, r, 1.0), r);
        sum[j] = __builtin_fma(r, q.sw, sum[j]);
      }
    } else if constexpr (NODES) {                               // not a smooth function of f across the window
      *failed |= 1u << k;
    } else {                                                    // cutoff differs between lanes / frequencies: masks
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = sfq[2 * j];
        const double d1 = f - q.c1;
        const double d2 = f + q.c1;
        const double D1 = __builtin_fma(d1, d1, q.wsq);
        const double D2 = __builtin_fma(d2, d2, q.wsq);
        const double m1 = (fabs(d1) < 750.0) ? 1.0 : 0.0;
        const double m2 = (fabs(d2) < 750.0) ? 1.0 : 0.0;
        const double num = __builtin_fma(m2, D1, m1 * D2);
        const double r = fdiv1(num, D1 * D2);
        sum[j] = __builtin_fma(r, q.sw, sum[j]);
        sum[j] = __builtin_fma(-(m1 + m2), q.sbase, sum[j]);
      }
    }
  }
  if constexpr (NODES) {                                        // raw line sums at the nodes; bsum travels separately
#pragma unroll
    for (int j = 0; j < NFC; ++j) awet[j] = sum[j];
    *bsum_out = bsum;
    return;
  }
#pragma unroll
  for (int j = 0; j < NFC; ++j) sum[j] -= bsum;
  // speed-dependent lines (ABH2O_SD): the resonant term inside |d1| < 10 w0 is the quadratic-speed-dependent
  // shape      Xc = (w0 - 1.5 w2 + i (d1 + 1.5 delta2)) / (w2 - i delta2),
  //            SD = 2 (1 - sqrt(pi) Xrt w(i Xrt)) / (w2 - i delta2),   Xrt = sqrt(Xc)
  // instead of the Lorentzian; outside it, and for the second term, the plain cutoff Lorentzians.
  const unsigned setC = (MWRT_ABLATE & 4) ? 0u : ((sd_eff | sd_extra) & all);
  for (unsigned m = setC; m; m &= m - 1u) {
    const int k = __builtin_ctz(m);
    const H2OLine q = h2o_line(M, k, pda, pvap, ti, tiln, ti2, shifted);
    const double w2 = M->h2o_w2[k] * pda * fexp(M->h2o_xw2[k] * tiln) + M->h2o_w2s[k] * pvap * fexp(M->h2o_xw2s[k] * tiln);
    const double delta2 = M->h2o_d2[k] * pda + M->h2o_d2s[k] * pvap;
    const cplx iden2 = crecip(cplx{w2, -delta2});              // 1 / (w2 - i delta2), once per (level, line)
    const double sdlim = (w2 > 0.0) ? 10.0 * q.w0 : -1.0;     // width2 == 0 at this level: plain Lorentz
    const double xre = q.w0 - 1.5 * w2, xim0 = 1.5 * delta2;
    LDS_RELOAD_FENCE();
    // pass 1: the cutoff Lorentzians, the resonant one masked out where the SD shape takes over
    const bool d1_in = (q.c1 - fmin < 750.0) && (fmax - q.c1 < 750.0) && (q.c1 - fmin > -750.0);
    const bool d2_in = fmax + q.c1 < 750.0 && fmin + q.c1 > -750.0;
    // half-sampled shape for this line and chunk?  (needs both Lorentz terms inside the cutoff: the common case)
    bool half = false;
    if constexpr (NFC == 16 && !NODES) half = sdw != nullptr && ((lm.h2o_sdint >> k) & 1u) && wave_all(d1_in && d2_in);
    if (wave_all(d1_in && d2_in)) {                                // both inside the cutoff everywhere (22 / 183 GHz lines)
      const double sbase2 = q.sbase + q.sbase;
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = sfq[2 * j];
        const double d1 = f - q.c1;
        const double d2 = f + q.c1;
        const double D1 = __builtin_fma(d1, d1, q.wsq);
        const double D2 = __builtin_fma(d2, d2, q.wsq);
        // (half-sampled: the odd slots keep their Lorentzian and get the interpolated difference in pass 2)
        const bool inner = fabs(d1) < sdlim && !(half && (j & 1) && j != 15);
        const double den12 = D1 * D2;
        double r = __builtin_amdgcn_rcp(den12);
        r = __builtin_fma(r, __builtin_fma(-den12, r, 1.0), r);
        const double num = inner ? D1 : D1 + D2;
        sum[j] = __builtin_fma(num * r, q.sw, sum[j]);
        sum[j] -= inner ? q.sbase : sbase2;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = sfq[2 * j];
        const double d1 = f - q.c1;
        const double d2 = f + q.c1;
        const double D1 = __builtin_fma(d1, d1, q.wsq);
        const double D2 = __builtin_fma(d2, d2, q.wsq);
        const double a1 = fabs(d1);
        const double m1 = (a1 < 750.0 && !(a1 < sdlim)) ? 1.0 : 0.0;
        const double m2 = (fabs(d2) < 750.0) ? 1.0 : 0.0;
        const double num = __builtin_fma(m2, D1, m1 * D2);
        const double r = fdiv1(num, D1 * D2);
        sum[j] = __builtin_fma(r, q.sw, sum[j]);
        sum[j] = __builtin_fma(-(m1 + m2), q.sbase, sum[j]);
      }
    }
    // pass 2: the SD resonant shape, frequency by frequency, only where some lane of the wave is inside
    // 10 half-widths (the branch is wave-uniform, so nothing of one frequency interleaves with the next)
    LDS_RELOAD_FENCE();
    auto sd_shape = [&](double d1) -> double {                  // Re SD at detuning d1
      const cplx xc = cmul(cplx{xre, d1 + xim0}, iden2);
      const cplx xrt = csqrt_principal(xc);
      const cplx w = dcerror_upper(-xrt.im, xrt.re);
      const cplx pxw = cmul(cplx{1.77245385090551603 * xrt.re, 1.77245385090551603 * xrt.im}, w);
      return __builtin_fma(2.0 * (1.0 - pxw.re), iden2.re, 2.0 * pxw.im * iden2.im);      // Re((2 - 2 pxw) iden2)
    };
    bool done = false;
    if constexpr (NFC == 16 && !NODES) {
      if (half) {
        done = true;
        // the chunk lies on one side of the line: the closest frequency is one of its ends
        const double dmin = ::fmin(fabs(sfq[0] - q.c1), fabs(sfq[2 * 15] - q.c1));
        if (wave_any(dmin < sdlim)) {
          double dn[SD_NODES];
#pragma unroll
          for (int n = 0; n < SD_NODES; ++n) {
            const int j = sd_node_slot(n);
            const double d1 = sfq[2 * j] - q.c1;
            const double sdre = sd_shape(d1);
            const double lres = fdiv1(q.w0, __builtin_fma(d1, d1, q.wsq));     // the Lorentzian the shape replaces
            dn[n] = sdre - lres;
            const double r1 = (fabs(d1) < sdlim) ? sdre - q.base : 0.0;
            sum[j] = __builtin_fma(q.s, r1, sum[j]);
          }
#pragma unroll
          for (int i = 0; i < SD_TARGETS; ++i) {
            const int j = 2 * i + 1;
            double dl = 0.0;
#pragma unroll
            for (int n = 0; n < SD_NODES; ++n) dl = __builtin_fma(sdw[i * SD_NODES + n], dn[n], dl);
            const bool inner = fabs(sfq[2 * j] - q.c1) < sdlim;
            sum[j] = __builtin_fma(q.s, inner ? dl : 0.0, sum[j]);
          }
        }
      }
    }
    if (!done) {
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double d1 = sfq[2 * j] - q.c1;
        const bool inner = fabs(d1) < sdlim;
        if (wave_any(inner)) {
          const double r1 = inner ? sd_shape(d1) - q.base : 0.0;
          sum[j] = __builtin_fma(q.s, r1, sum[j]);
        }
      }
    }
  }
  const bool dry = !(L.rho > 0.0);
#pragma unroll
  for (int j = 0; j < NFC; ++j) {
    const double f2 = sfq[2 * j + 1];
    awet[j] = dry ? 0.0 : (3.183e-05 * den * sum[j] + con0) * f2;
  }
}

// ---------------------------------------------------------------------------------------------
// K1b: O2 lines + non-resonant + N2 continuum (O2AbsModel.o2_absorption / N2AbsModel [EXT])
//   S (f/F)^2 [ (w g + d1 Y)/D1 + (w g - d2 Y)/D2 ]  with one reciprocal per line and frequency
// ---------------------------------------------------------------------------------------------
// fma(table value, lane value, table value): a v_fma_f64 reads one scalar operand at most, so one of the two table values
// has to sit in a vector register pair, and the compiler takes it there with two v_mov_b32.  Table values arrive in scalar
// registers (s_load), and gfx950 moves such a pair in ONE instruction: the addend is handed over by a v_mov_b64, and the
// FMA accumulates into the registers it wrote.  Same operands, same operation, same bits; one VALU instruction fewer per
// such FMA.  (FUSED: the fused kernel's set-ups only; the other kernels keep the compiler's form.)
template <bool FUSED>
__device__ __forceinline__ double table_addend(double s) {
  if constexpr (FUSED) {
    double v;
    asm("v_mov_b64 %0, %1" : "=v"(v) : "s"(s));
    return v;
  } else {
    return s;
  }
}

struct O2Line {            // per-(level, line) quantities, frequency independent (all carry HALF the line's weight:
  double c1, df2;          //  the common factor 2 of P and Q is applied once, in the final scale)
  double P, Q;             //  n1/D1 + n2/D2 = 2 (f^2 P + Q) / (D1 D2),  P = a + c b,  Q = (c^2 + w^2)(a - c b)
  double cc;               //  c^2 + w^2
  double dnu;
};

template <int NFC, bool NODES = false, bool GROUPED = false>
__device__ __forceinline__ void dry_absorb(cmodel M, const LevelState& L, const double* sfq /*LDS: {f, f^2} per slot*/,
                                           const LineMasks& lm, double (&adry)[NFC], unsigned long long excl = 0ull,
                                           const double* init_sum = nullptr, unsigned long long* failed = nullptr) {
  const double temp = L.t;
  const double pres = L.p;
  const double th = fdiv(300.0, temp);
  const double th1 = th - 1.0;
  const double lnth = flog(th);
  const double b = fexp(M->o2_x * lnth);
  const double preswv = fdiv(L.rho * temp, M->o2_pvap_div);
  const double presda = pres - preswv;
  const double den = 0.001 * (presda * b + M->o2_wv_factor * preswv * th);
  const double dens = 0.001 * (presda + M->o2_wv_factor * preswv) * th;
  const double dfnr = M->o2_wb300 * den;
  const double pe2 = den * den;
  const bool second = M->o2_mix_mode != 0;
  const double ymul = second ? den : 0.001 * pres * b;
  const bool line1_dens = !second && M->o2_line1_dens;

  double sum[NFC];
#pragma unroll
  for (int j = 0; j < NFC; ++j) sum[j] = init_sum ? init_sum[j] : 0.0;

  // With d1 = f - c, d2 = f + c, D = d^2 + w^2, n1 = a + d1 b, n2 = a - d2 b the two terms of a line
  // share one reciprocal and the numerator collapses to a polynomial in f^2:
  //   n1/D1 + n2/D2 = (f^2 P + Q) / (D1 D2),  P = 2 (a + c b),  Q = 2 (c^2 + w^2)(a - c b)
  long long be_prev = -1;
  double ebe = 1.0;
  auto line_setup = [&](int k) -> O2Line {
    const auto& R = M->o2r[k];
    // A set-up reads its record in four scalar loads, each placed in front of its first use with a wait behind it: four
    // round trips to the scalar cache per line, and a SIMD holds only three of these waves to cover them.  Asking for BE,
    // W300, Y0 and Y1 here makes them ONE eight-dword load at the top of the set-up (they are adjacent in O2Rec), three
    // round trips per line.  The fused kernel only; more of the record up front costs it scratch.
    if constexpr (GROUPED) asm volatile("" :: "s"(R.be), "s"(R.w300), "s"(R.y0), "s"(R.y1));
    // slope and offset are both table values: the offset goes to the vector side in one move (table_addend)
    const double y = ymul * __builtin_fma(R.y1, th1, table_addend<GROUPED>(R.y0));
    double dnu = 0.0, gfac = 1.0;
    if (second) {
      dnu = pe2 * __builtin_fma(R.dnu1, th1, table_addend<GROUPED>(R.dnu0));
      gfac = __builtin_fma(pe2, __builtin_fma(R.g1, th1, table_addend<GROUPED>(R.g0)), 1.0);
    }
    const double df = R.w300 * ((k == 0 && line1_dens) ? dens : den);
    // N- / N+ partners share BE: the exponential is redone only when the table value changes
    // (compared as bit patterns so the test stays on the scalar unit)
    const long long be_bits = __builtin_bit_cast(long long, R.be);
    if (be_bits != be_prev) { ebe = fexp(-R.be * th1); be_prev = be_bits; }
    const double str = R.s300rf2 * ebe;                               // S300 / F^2 (the f^2 is applied at the end)
    O2Line q;
    q.dnu = dnu;
    q.c1 = R.f + dnu;
    q.df2 = df * df;
    const double a = (str * df) * gfac;
    const double cb = q.c1 * (str * y);
    q.cc = __builtin_fma(q.c1, q.c1, q.df2);
    q.P = a + cb;
    q.Q = q.cc * (a - cb);
    return q;
  };

  const int nl = M->n_o2;
  const unsigned long long all = o2_lines_all(nl) & ~excl;
  // loop A: far lines -- polynomial denominator; a line whose shift |dnu| exceeds the allowance at any
  // level of this wave is handed to loop B
  unsigned long long near = ~lm.o2_far & all;
  const unsigned long long setA = (MWRT_ABLATE & 1) ? 0ull : o2_far_set(lm, all);
  // ... four lines at a time (far_quad_accumulate); the count mod 4 left over joins loop B
  const unsigned long long setV = o2_vfar_set(lm, setA, NODES);           // very far lines: one Taylor polynomial (vfar_add)
  const unsigned long long setQ = o2_quad_set(lm, setA, NODES);
  const unsigned long long leftA = lowest_bits(setQ, __builtin_popcountll(setQ) & 3);
  const unsigned long long leftP = (__builtin_popcountll(leftA) >= 2) ? lowest_bits(leftA, 2) : 0ull;   // ... two of them as a pair
  near |= leftA & ~leftP;
  auto far_setup = [&](int k, FarLine& fl) {
    const O2Line q = line_setup(k);
    double P = q.P, Q = q.Q;
    if (!NODES && second && !wave_all(fabs(q.dnu) < FAR_SHIFT_GHZ)) { near |= 1ull << k; P = 0.0; Q = 0.0; }
    fl.P = P; fl.Q = Q;
    fl.A2 = 2.0 * __builtin_fma(-q.c1, q.c1, q.df2);
    fl.Bc = q.cc * q.cc;
  };
  if (setV) {
    double acc[VF_TERMS];
#pragma unroll
    for (int j = 0; j < VF_TERMS; ++j) acc[j] = 0.0;
    for (unsigned long long m = setV; m; m &= m - 1ull) {
      FarLine q;
      far_setup(__builtin_ctzll(m), q);
      vfar_add(q, lm.vf_u0, lm.vf_h, acc);
    }
    LDS_RELOAD_FENCE();
    vfar_eval<NFC>(sfq, lm.vf_invh, -lm.vf_u0 * lm.vf_invh, acc, sum);
  }
  if constexpr (GROUPED) far_groups_accumulate<NFC>(sfq, setQ & ~leftA, far_setup, sum);
  else for (unsigned long long m = setQ & ~leftA; m;) {
    FarLine q0, q1, q2, q3;
    far_setup(__builtin_ctzll(m), q0); m &= m - 1ull;
    far_setup(__builtin_ctzll(m), q1); m &= m - 1ull;
    far_setup(__builtin_ctzll(m), q2); m &= m - 1ull;
    far_setup(__builtin_ctzll(m), q3); m &= m - 1ull;
    LDS_RELOAD_FENCE();
    far_quad_accumulate<NFC>(sfq, q0, q1, q2, q3, sum);
  }
  if (leftP) {
    FarLine q0, q1;
    unsigned long long m = leftP;
    far_setup(__builtin_ctzll(m), q0); m &= m - 1ull;
    far_setup(__builtin_ctzll(m), q1);
    LDS_RELOAD_FENCE();
    far_pair_accumulate<NFC>(sfq, q0, q1, sum);
  }
  // loop B: lines next to a chunk frequency -- D1, D2 formed from the detunings directly (no cancellation)
  if (MWRT_ABLATE & 1) near = 0ull;
  be_prev = -1;
  for (unsigned long long m = near; m; m &= m - 1ull) {
    const int k = __builtin_ctzll(m);
    const O2Line q = line_setup(k);
    LDS_RELOAD_FENCE();
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
      const double f = sfq[2 * j], f2 = sfq[2 * j + 1];
      const double d1 = f - q.c1;
      const double d2 = f + q.c1;
      const double D1 = __builtin_fma(d1, d1, q.df2);
      const double D2 = __builtin_fma(d2, d2, q.df2);
      const double den12 = D1 * D2;
      double r = __builtin_amdgcn_rcp(den12);
      r = __builtin_fma(r, __builtin_fma(-den12, r, 1.0), r);
      sum[j] = __builtin_fma(__builtin_fma(f2, q.P, q.Q), r, sum[j]);
    }
  }
  if constexpr (NODES) {                                        // raw half-weight line sums at the nodes
#pragma unroll
    for (int j = 0; j < NFC; ++j) adry[j] = sum[j];
    (void)failed;
    return;
  }
  const double scale2 = 2.0 * M->o2_coef * presda * th * th * th;     // the 2 of P and Q
  // N2 collision-induced continuum (ABSN2): p^2 f^2 th^m
  const double pn2 = M->n2_ptot ? pres : L.pdry;
  const double n2c = M->n2_n * M->n2_l * pn2 * pn2 * fexp(M->n2_m * lnth);
  const double nr0 = 0.5 * M->o2_nonres * dfnr;
  const double dfnr2 = dfnr * dfnr;
#pragma unroll
  for (int j = 0; j < NFC; ++j) {
    const double f2 = sfq[2 * j + 1];
    const double hnonres = fdiv(nr0 * f2, th * (f2 + dfnr2));          // half the non-resonant term
    double o2 = scale2 * __builtin_fma(sum[j], f2, hnonres);
    o2 = fmax(o2, 0.0);
    adry[j] = o2 + n2c * sfq[2 * NFC + 2 + j] * f2;          // N2 frequency-dependence factor, per slot
  }
}

// ---------------------------------------------------------------------------------------------
// Opt-in physics the reference leaves at pyrtlib's defaults: cloud liquid / ice
// absorption (cloudy=True + init_cloudy) and spherical refracted ray tracing (ray_tracing=True).
// Only the OPT instantiations of the fused kernel contain this code; the clear-sky kernels are untouched.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ cplx clog_(cplx w) {       // principal complex logarithm
  return {0.5 * flog(__builtin_fma(w.re, w.re, w.im * w.im)), atan2(w.im, w.re)};
}

// RTEquation.cloudy_absorption + LiqAbsModel.liquid_water_absorption [EXT]: Np/km at one level.
// The frequency-independent part of the liquid model is built once per level (CloudLevel), the per-frequency
// part is a handful of complex operations; ice is (8.18645 / wavelength[cm]) * deni * 0.000959553 dB/km.
struct CloudLevel {
  int mode;                      // liq_mode of the model
  double eps0;                   // static dielectric constant
  // mode 0 (Liebe, Hufford & Manabe 1991 / MPM93 double Debye):  a = eps1, b = 1/fp, c = 1/fs
  // mode 1 (Rosenkranz 2015: Patek 2009 static constant, Ellison 2007 Debye term, B-band term):
  //         a = delta, b = sd, c = delta_B, z1 and 1/cnorm complex
  double a, b, c;
  cplx z1, icnorm;
};
constexpr double CLOUD_KICE = 8.18645 * 0.000959553 * (0.1 * 2.302585092994045684) / 29.9792458;

__device__ __forceinline__ CloudLevel cloud_level(cmodel M, double tk) {
  const int mode = M->liq_mode;
  double eps0, a, b, c3;
  cplx z1 = {0.0, 0.0}, icnorm = {0.0, 0.0};
  if (mode == 0) {
    const double theta1 = 1.0 - fdiv(300.0, tk);
    eps0 = 77.66 - 103.3 * theta1;
    a = 0.0671 * eps0;
    const double fp = (316.0 * theta1 + 146.4) * theta1 + 20.2;
    b = fdiv(1.0, fp);
    c3 = fdiv(1.0, 39.8 * fp);
  } else {
    const double tc = tk - 273.15;
    const double lth = flog(fdiv(300.0, tk));
    eps0 = -43.7527 * fexp(0.05 * lth) + 299.504 * fexp(1.47 * lth) - 399.364 * fexp(2.11 * lth) + 221.327 * fexp(2.31 * lth);
    a = 80.69715 * fexp(-tc * (1.0 / 226.45));
    b = 1164.023 * fexp(fdiv(-651.4728, tc + 133.07));
    c3 = 4.008724 * fexp(-tc * (1.0 / 103.05));
    const double f1 = 10.46012 + tc * (0.1454962 + tc * (0.063267156 + tc * 0.00093786645));
    z1 = cplx{-0.75 * f1, f1};
    icnorm = crecip(clog_(cdiv(cplx{-4500.0, 2000.0}, z1)));      // 1/cnorm; 1/conj(cnorm) is its conjugate
  }
  return CloudLevel{mode, eps0, a, b, c3, z1, icnorm};
}

// liquid absorption for water content `denl` [g m-3] at frequency f [GHz]
__device__ __forceinline__ double liquid_abs(const CloudLevel& c, double f, double denl) {
  cplx eps;
  if (c.mode == 0) {
    const double eps2 = 3.52;
    const cplx t1 = cdiv(cplx{c.eps0 - c.a, 0.0}, cplx{1.0, f * c.b});
    const cplx t2 = cdiv(cplx{c.a - eps2, 0.0}, cplx{1.0, f * c.c});
    eps = cplx{t1.re + t2.re + eps2, t1.im + t2.im};
  } else {
    const cplx z2 = {-4500.0, 2000.0};
    const double hdelta = 0.5 * c.c;
    const cplx kap0 = cdiv(cplx{0.0, -c.a * f}, cplx{c.b, f});                   // -delta z / (sd + z), z = i f
    const cplx lp = clog_(cdiv(cplx{-z2.re, f - z2.im}, cplx{-c.z1.re, f - c.z1.im}));
    const cplx lj = clog_(cdiv(cplx{-z2.re, f + z2.im}, cplx{-c.z1.re, f + c.z1.im}));
    const cplx chip = cmul(cplx{hdelta * lp.re, hdelta * lp.im}, c.icnorm);
    const cplx chij = cmul(cplx{hdelta * lj.re, hdelta * lj.im}, cplx{c.icnorm.re, -c.icnorm.im});
    eps = cplx{c.eps0 + (kap0.re + (chip.re + chij.re - c.c)), kap0.im + (chip.im + chij.im)};
  }
  const cplx re = cdiv(cplx{eps.re - 1.0, eps.im}, cplx{eps.re + 2.0, eps.im});
  return -0.06286 * re.im * f * denl;
}

// RTEquation.refractivity [EXT] (Thayer 1974): refractive index at one level
__device__ __forceinline__ double thayer_refindex(double p, double tk, double e) {
  const double pa = p - e, tc = tk - 273.16, tk2 = tk * tk, tc2 = tc * tc;
  const double rza = 1.0 + pa * (5.79e-07 * (1.0 + 0.52 / tk) - (0.00094611 * tc) / tk2);
  const double rzw = 1.0 + 1650.0 * (e / (tk * tk2)) * (1.0 - 0.01317 * tc + 0.000175 * tc2 + 1.44e-06 * (tc2 * tc));
  const double wetn = (64.79 * (e / tk) + 377600.0 * (e / tk2)) * rzw;
  const double dryn = 77.6036 * (pa / tk) * rza;
  return 1.0 + (dryn + wetn) * 1e-06;
}

// O3AbsModel.o3_absorption [EXT, recalled from Rosenkranz's o3abs -- unverified; the line list is data, include/mwrt.h
// mwrt_model_desc.n_x]: the extra trace species joins the DRY absorption of this level for the chunk's frequencies
// (RTEquation.clearsky_absorption(..., o3n) [EXT]).  Generic Van Vleck-Weisskopf lines with a Voigt half width; one
// reciprocal per line and frequency.  Opt-in path, not tuned.
template <int NFC>
__device__ __forceinline__ void x_absorb(cmodel M, double tk, double p, double numden, const double* sfq, double (&adry)[NFC]) {
  const double ti = fdiv(M->x_reft, tk);
  const double tiln = flog(ti);
  const double qvinv = (M->x_qvib_t > 0.0) ? 1.0 - fexp(-fdiv(M->x_qvib_t, tk)) : 1.0;
  const double sq = 4.3e-07 * fsqrt(fdiv(tk, M->x_mass));
  double sum[NFC];
#pragma unroll
  for (int j = 0; j < NFC; ++j) sum[j] = 0.0;
  const int nx = M->n_x;
  for (int k = 0; k < nx; ++k) {
    const double fl = M->x_fl[k];
    const double wc = M->x_w[k] * p * fexp(M->x_x[k] * tiln);
    const double bd = sq * fl;
    const double w = 0.5346 * wc + fsqrt(__builtin_fma(0.2166 * wc, wc, 0.6931 * (bd * bd)));
    const double wsq = w * w;
    const double sw = (M->x_s1[k] * fexp(M->x_b[k] * (1.0 - ti))) * fdiv(w, fl * fl);     // the f^2 of (f/FL)^2 is applied at the end
    LDS_RELOAD_FENCE();
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
      const double f = sfq[2 * j];
      const double d1 = f - fl, d2 = f + fl;
      const double D1 = __builtin_fma(d1, d1, wsq), D2 = __builtin_fma(d2, d2, wsq);
      const double den12 = D1 * D2;
      double r = __builtin_amdgcn_rcp(den12);
      r = __builtin_fma(r, __builtin_fma(-den12, r, 1.0), r);
      sum[j] = __builtin_fma((D1 + D2) * r, sw, sum[j]);
    }
  }
  const double pref = ((M->x_coef * numden) * qvinv) * fexp(2.5 * tiln);
#pragma unroll
  for (int j = 0; j < NFC; ++j) adry[j] = __builtin_fma(pref * sfq[2 * j + 1], sum[j], adry[j]);
}

}  // namespace mwrt
