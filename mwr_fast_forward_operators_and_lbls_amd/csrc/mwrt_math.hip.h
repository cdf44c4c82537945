// mwrt_math.hip.h -- device arithmetic shared by every kernel unit: the build switches that change code, division /
// exp / log / tanh / sqrt on the kernels' bounded arguments, wave votes, the Planck function, complex helpers, the
// workgroup sum and the fences that pin an instruction order.  fp64 throughout; nothing here knows a table or a kernel.
#pragma once
#include "mwrt_args.hip.h"      // MWRT_PHASE_CLOCK's default (MWRT_STAMP follows it), WAVE

namespace mwrt {

// n / d for the small operands of the K2 work split (see LaunchGeom): one v_mul_hi_u32
__device__ __forceinline__ int div_small(int n, int d, unsigned magic) {
  return d == 1 ? n : (int)__umulhi((unsigned)n, magic);
}

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
#ifndef MWRT_EXACT_DIV
#define MWRT_EXACT_DIV 0
#endif
// timing-only ablation builds (tools/ablate.sh): bit 1 skips the O2 line loop, 2 the H2O Lorentz
// loop, 4 the speed-dependent loop, 8 the K2 integration, 16 the layer step of the TAU absorption kernels, 32 their
// stores, 64 the scalar loads of their interpolation weights.  Always 0 in the shipped library.
#ifndef MWRT_ABLATE
#define MWRT_ABLATE 0
#endif
// Issue priority by phase.  A SIMD issues from its OLDEST ready wave first, so of the three or four workgroups a CU holds the
// first one dispatched runs almost as if alone and the last one gets the gaps: in the single resident round of the headline
// shape (1000 workgroups, four per CU, all started within 0.3 us) the phase stamps of a -DMWRT_PHASE_CLOCK=1 build show the
// four workgroups of every CU leaving at 70 / 81 / 108 / 111 us -- the last ones run their final 30 us with one or two waves
// per SIMD, latency-bound.  s_setprio beats age: a wave in an EARLIER phase gets the higher priority (3 water lines,
// 2 oxygen lines, 1 layer step + first RTE pass, 0 second RTE pass), so the laggards of a SIMD catch up at every phase
// change and all waves finish together (88 ... 101 us): 116 -> 105 us.  -DMWRT_NO_SETPRIO=1 builds without it (A/B timing).
#ifndef MWRT_NO_SETPRIO
#define MWRT_NO_SETPRIO 0
#endif
#if MWRT_NO_SETPRIO
#define MWRT_SETPRIO(n) do { } while (0)
#else
#define MWRT_SETPRIO(n) __builtin_amdgcn_s_setprio(n)
#endif
#if MWRT_PHASE_CLOCK
#define MWRT_STAMP(k) do { if (A.phase && lane == 0) A.phase[((int64_t)blockIdx.x * 4 + wave) * 10 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define MWRT_STAMP(k) do { } while (0)
#endif
// k_tb_fused's occupancy pin for its EXTRAS instantiations (see the kernel, csrc/mwrt_fused.hip.h)
#ifndef MWRT_MIN_WAVES
#define MWRT_MIN_WAVES 1
#endif

// x / d with v_rcp_f64 + two Newton steps (~1.5 ulp; parity bar is 1e-6 K, budget 0.01 K).
__device__ __forceinline__ double fdiv(double x, double d) {
#if MWRT_EXACT_DIV
  return x / d;
#else
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  return x * r;
#endif
}

// exp(x) for the kernels' bounded arguments: Cody-Waite reduction + a degree-11 polynomial on |r| <= ln2/2
// (1 + r + r^2 g(r), g fitted at the Chebyshev nodes of the interval: 1.7e-17 relative; the degree-13 Taylor
// series it replaces had 4e-18 and two more steps), scaled by v_ldexp_f64 (which also gives the right 0 / inf at
// the range ends).
// ocml's exp spends two VALU instructions per Horner step (v_mov of the 64-bit constant + v_fmac);
// here each constant rides in an SGPR pair (materialised by s_mov, off the VALU port), so a step
// is ONE v_fma_f64.  ~19 VALU instead of ~35; max relative error measured < 4e-16.
#define MWRT_FMA_SC(p, r, c) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(r), "s"(c))
// The LEADING coefficient of such a Horner chain is the one operand that has to sit in a vector register (the first
// step reads it as `p`), and the compiler re-materialises it with a v_mov_b64 at every evaluation.  A loop that
// evaluates the polynomial per trip takes the coefficient as an argument instead and holds it in a register across the
// loop (loop_invariant_vgpr): same constant, same chain, one VALU instruction fewer per evaluation.
__device__ __forceinline__ double loop_invariant_vgpr(double c) {
  asm volatile("" : "+v"(c));                        // opaque: cannot be re-materialised inside the loop
  return c;
}
constexpr double FEXP_C0 = 2.5100569275813683e-08;
__device__ __forceinline__ double fexp(double x, double c0 = FEXP_C0) {
#if MWRT_EXACT_DIV
  return exp(x);
#else
  const double k = __builtin_rint(x * 1.4426950408889634074);
  double r = __builtin_fma(k, -6.93147180369123816490e-01, x);
  r = __builtin_fma(k, -1.90821492927058770002e-10, r);
  double p = c0;
  MWRT_FMA_SC(p, r, 2.762032742826824e-07);
  MWRT_FMA_SC(p, r, 2.75572680728901e-06);
  MWRT_FMA_SC(p, r, 2.4801520792572694e-05);
  MWRT_FMA_SC(p, r, 0.00019841269863303223);
  MWRT_FMA_SC(p, r, 0.0013888888917538296);
  MWRT_FMA_SC(p, r, 0.008333333333330011);
  MWRT_FMA_SC(p, r, 0.04166666666662348);
  MWRT_FMA_SC(p, r, 0.16666666666666669);
  MWRT_FMA_SC(p, r, 0.5000000000000001);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  return __builtin_amdgcn_ldexp(p, (int)k);
#endif
}

// (2 atanh(s)/s - 2)/z = 2/3 + 2z/5 + ..., z = s^2 <= 0.1716^2, as a degree-6 polynomial fitted at the Chebyshev nodes of
// the interval: 2 atanh(s)/s to 4.6e-18 relative in 7 steps (the Taylor series needs 10 for 5e-17)
__device__ __forceinline__ double two_atanh_tail(double z) {
  double p = 0.14616878919029822;
  MWRT_FMA_SC(p, z, 0.15331686868638428);
  MWRT_FMA_SC(p, z, 0.1818289017031397);
  MWRT_FMA_SC(p, z, 0.22222211120449298);
  MWRT_FMA_SC(p, z, 0.2857142862606338);
  MWRT_FMA_SC(p, z, 0.3999999999989931);
  MWRT_FMA_SC(p, z, 0.666666666666667);
  return p;
}

// log(x), x > 0 finite and normal (layer ratios of positive absorption coefficients): frexp to
// m in [sqrt(1/2), sqrt(2)), s = (m-1)/(m+1), log m = 2 s (1 + z/3 + z^2/5 + ...) = s (2 + z two_atanh_tail(z)), z = s^2
// (|s| <= 0.1716).  Keeps full RELATIVE accuracy as x -> 1, which is what the
// log-mean of two nearly equal levels needs.  ~33 VALU against ~50 for ocml's log.
__device__ __forceinline__ double flog(double x) {
#if MWRT_EXACT_DIV
  return log(x);
#else
  int e = __builtin_amdgcn_frexp_exp(x);
  double m = __builtin_amdgcn_frexp_mant(x);            // [0.5, 1)
  const bool lo = m < 0.70710678118654752440;
  m = lo ? m + m : m;
  e = lo ? e - 1 : e;
  const double num = m - 1.0, den = m + 1.0;
  double r = __builtin_amdgcn_rcp(den);
  r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
  r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
  const double s = num * r;
  const double z = s * s;
  const double p = two_atanh_tail(z);                   // (2 atanh(s)/s - 2) / z
  const double ed = (double)e;
  const double lm = __builtin_fma(s * z, p, s + s);     // log(m)
  return __builtin_fma(ed, 6.93147180369123816490e-01, __builtin_fma(ed, 1.90821492927058770002e-10, lm));
#endif
}

// exp(x) for |x| <= 1/8 with no range reduction: 1 + x + x^2 g(x), g of degree 7 fitted at the Chebyshev nodes
// (2.2e-18 relative).  9 VALU.
// Thin layers (tau * airmass <= 1/8) are the rule for the K-band channels at every level and angle.
constexpr double EXP_SMALL_X = 0.125;
constexpr double FEXP_SMALL_C0 = 2.756514908613403e-06;
__device__ __forceinline__ double fexp_small(double x, double c0 = FEXP_SMALL_C0) {
  double p = c0;
  MWRT_FMA_SC(p, x, 2.4810200365624755e-05);
  MWRT_FMA_SC(p, x, 0.00019841269076602318);
  MWRT_FMA_SC(p, x, 0.001388888804772704);
  MWRT_FMA_SC(p, x, 0.008333333333357229);
  MWRT_FMA_SC(p, x, 0.04166666666692954);
  MWRT_FMA_SC(p, x, 0.16666666666666666);
  MWRT_FMA_SC(p, x, 0.4999999999999999);
  p = __builtin_fma(p, x, 1.0);
  return __builtin_fma(p, x, 1.0);
}

// tanh(x/2) = (1 - e^-x) / (1 + e^-x) for 0 <= x <= 1/8: x (1/2 + u g(u)), u = x^2, g of degree 3 fitted at the Chebyshev
// nodes of [0, 1/64] (6e-17 relative).  6 VALU; in the thin-layer RTE step it replaces 1 - E, 1 + E and their quotient (9 issue slots), and has none
// of the cancellation of 1 - E.
constexpr double FTANH_HALF_SMALL_C0 = 4.257889640378761e-05;
__device__ __forceinline__ double ftanh_half_small(double x, double c0 = FTANH_HALF_SMALL_C0) {
  const double u = x * x;
  double p = c0;
  MWRT_FMA_SC(p, u, -0.0004216256671577941);
  MWRT_FMA_SC(p, u, 0.004166666662552237);
  MWRT_FMA_SC(p, u, -0.04166666666666466);
  p = __builtin_fma(p, u, 0.5);
  return p * x;
}

// ... and for |x| <= 1/64: exp to degree 6 (truncation 9e-18), tanh(x/2) through x^7 (next term 3e-21 relative). 7 + 5 VALU.
constexpr double EXP_TINY_X = 0.015625;
__device__ __forceinline__ double fexp_tiny(double x) {
  double p = 1.3888888888888889e-03;                 // 1/6!
  MWRT_FMA_SC(p, x, 8.3333333333333332e-03);         // 1/5!
  MWRT_FMA_SC(p, x, 4.1666666666666664e-02);         // 1/4!
  MWRT_FMA_SC(p, x, 1.6666666666666666e-01);         // 1/3!
  p = __builtin_fma(p, x, 0.5);
  p = __builtin_fma(p, x, 1.0);
  return __builtin_fma(p, x, 1.0);
}
__device__ __forceinline__ double ftanh_half_tiny(double x) {
  const double u = x * x;
  double p = -4.2162698412698413e-04;                // -17/40320
  MWRT_FMA_SC(p, u, 4.1666666666666666e-03);         // 1/240
  MWRT_FMA_SC(p, u, -4.1666666666666664e-02);        // -1/24
  p = __builtin_fma(p, u, 0.5);
  return p * x;
}

// Wave votes straight from the comparison mask: HIP's __all / __any take an int, and the compiler materialises it
// (v_cndmask 0/1, v_cmp_ne) before comparing with exec -- two VALU instructions and a VALU -> SALU hazard per vote.
typedef unsigned long long wmask;
__device__ __forceinline__ bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// ... and a conjunction of comparisons as the AND of their masks on the scalar unit (pass each comparison separately)
__device__ __forceinline__ wmask wballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
template <class... B>
__device__ __forceinline__ bool wave_all_of(B... b) { return (wballot(b) & ...) == wballot(true); }

// max over the 16 lanes of a DPP row (lanes 16k .. 16k+15), delivered to all of them: row_ror 8, 4, 2, 1.
// Four VALU instructions, no LDS crossbar.
__device__ __forceinline__ float row16_max(float m) {
  m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x128, 0xf, 0xf, false)));
  m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x124, 0xf, 0xf, false)));
  m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x122, 0xf, 0xf, false)));
  m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x121, 0xf, 0xf, false)));
  return m;
}
// (K2_SORT_MIN_SEGLEN, the shortest segment whose items are dealt out sorted: mwrt_plan.h -- the row stride depends on it)

// Planck function in pyrtlib's units, B = 1 / (exp(x) - 1), x = h f / (k T).  In the microwave x is a few
// 1e-3: when the whole wave has x <= 1/32, B = (1/x) * x/(e^x - 1) with the Bernoulli series
// x/(e^x - 1) = 1 - x/2 + x^2/12 - x^4/720 + x^6/30240 (next term 8e-19) and 1/x = (k T / h) * (1/f) from
// per-level and per-frequency factors the caller holds: 8 VALU, no exp, no reciprocal, and none of the
// cancellation of exp(x) - 1 (which costs pyrtlib itself ~3e-14 relative; far below the parity bar).
constexpr double PLANCK_SMALL_X = 0.03125;
__device__ __forceinline__ double planck_b(double x, double inv_x) {
  if (wave_all_of(x <= PLANCK_SMALL_X, x > 0.0)) {
    const double u = x * x;
    double g = 3.3068783068783071e-05;                 // 1/30240
    MWRT_FMA_SC(g, u, -1.3888888888888889e-03);        // -1/720
    MWRT_FMA_SC(g, u, 8.3333333333333329e-02);         // 1/12
    g = __builtin_fma(g, u, 1.0);
    g = __builtin_fma(x, -0.5, g);
    return g * inv_x;
  }
  return fdiv(1.0, fexp(x) - 1.0);
}

// inner-loop variant: one Newton step (v_rcp_f64 is good to ~2^-23, so ~2^-46 ~ 1.4e-14 relative)
__device__ __forceinline__ double fdiv1(double x, double d) {
#if MWRT_EXACT_DIV
  return x / d;
#else
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
  return x * r;
#endif
}

// Frequencies are wave-uniform.  Held in SGPRs, {f, f^2} x 14 is 56 scalar registers and the
// allocator spills them into VGPR lanes (v_readlane per use).  They live in LDS instead and are
// re-read by broadcast each line iteration; the fence stops the compiler hoisting the reads
// back into (vector) registers across the line loop.
#define LDS_RELOAD_FENCE() asm volatile("" ::: "memory")
// A wave-uniform if / else whose sides are both free of side effects gets flattened by the optimiser into "evaluate
// both, select" -- the opposite of what a wave vote is for.  An empty volatile asm cannot be speculated: placed at the
// top of each side it keeps the branch a branch.
#define KEEP_BRANCH() asm volatile("")
// full scheduling barrier: the stages of a loop pipelined by hand stay in the order written (far_quad_accumulate)
#define MWRT_STAGE() __builtin_amdgcn_sched_barrier(0)

struct cplx { double re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx cadd(cplx a, double r) { return {a.re + r, a.im}; }
// 1 / b for complex b (one real reciprocal): the speed-dependent shape divides twice by the same
// per-(level, line) quantity, so the loop body multiplies by this instead
__device__ __forceinline__ cplx crecip(cplx b) {
  const double d = __builtin_fma(b.re, b.re, b.im * b.im);
#if MWRT_EXACT_DIV
  const double r = 1.0 / d;
#else
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
  r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
#endif
  return {b.re * r, -b.im * r};
}
__device__ __forceinline__ cplx cdiv(cplx a, cplx b) { return cmul(a, crecip(b)); }
// sqrt(x), x > 0 finite and far from the denormal range: v_rsq_f64 seed (~2^-23) + one coupled
// Newton step on (g ~ sqrt x, h ~ 1/(2 sqrt x)) -> ~2^-45 relative
__device__ __forceinline__ double fsqrt(double x) {
#if MWRT_EXACT_DIV
  return sqrt(x);
#else
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y;
  const double h = 0.5 * y;
  return __builtin_fma(__builtin_fma(-g, g, x), h, g);      // x == 0 gives NaN: callers never use that lane
#endif
}
__device__ __forceinline__ cplx csqrt_principal(cplx z) {
  const double r = fsqrt(__builtin_fma(z.re, z.re, z.im * z.im));
  // one square root and one division, selected by the sign of Re z:
  //   Re z >= 0: a = sqrt((r + Re z)/2), result (a, Im z / 2a);  Re z < 0: b = sqrt((r - Re z)/2), result (|Im z| / 2b, +-b)
  const bool pos = z.re >= 0.0;
  const double a = fsqrt(0.5 * (r + fabs(z.re)));
  const double q = fdiv1(pos ? z.im : fabs(z.im), a + a);    // z == 0 is outside the SD shape's domain (Re Xc > 0)
  return pos ? cplx{a, q} : cplx{q, copysign(a, z.im)};
}

// Rosenkranz DCERROR [EXT]: Hui, Armstrong & Wray (1978) rational approximation of the complex
// error function, upper half plane (y >= 0 always holds here: y = Re(principal sqrt)).
__device__ __forceinline__ cplx dcerror_upper(double x, double y) {
  const double a0 = 122.607931777104326, a1 = 214.382388694706425, a2 = 181.928533092181549,
               a3 = 93.155580458138441, a4 = 30.180142196210589, a5 = 5.912626209773153,
               a6 = 0.564189583562615;
  const double b0 = 122.607931773875350, b1 = 352.730625110963558, b2 = 457.334478783897737,
               b3 = 348.703917719495792, b4 = 170.354001821091472, b5 = 53.992906912940207,
               b6 = 10.479857114260399;
  const cplx zh = {fabs(y), -x};
  // Both polynomials have REAL coefficients: at a complex point they cost two real FMAs per coefficient (instead of
  // the four of a complex Horner step) through the quadratic z^2 = r z - s, r = 2 Re z, s = |z|^2:
  //   b_n = a_n,  b_{n-1} = a_{n-1} + r b_n,  b_k = a_k + r b_{k+1} - s b_{k+2},  p(z) = a_0 + z b_1 - s b_2
  // (agrees with complex Horner to < 5e-15 relative over |z| <= 100; the rational itself is Hui's, ~1e-6).
  const double r = zh.re + zh.re;
  const double ms = -__builtin_fma(zh.re, zh.re, zh.im * zh.im);
  auto step = [&](double c, double b1, double b2) -> double { return __builtin_fma(r, b1, __builtin_fma(ms, b2, c)); };
  double n2 = a6, n1 = __builtin_fma(r, a6, a5), nt;
  nt = step(a4, n1, n2); n2 = n1; n1 = nt;
  nt = step(a3, n1, n2); n2 = n1; n1 = nt;
  nt = step(a2, n1, n2); n2 = n1; n1 = nt;
  nt = step(a1, n1, n2); n2 = n1; n1 = nt;
  const cplx as = {__builtin_fma(zh.re, n1, __builtin_fma(ms, n2, a0)), zh.im * n1};
  double d2 = 1.0, d1 = r + b6, dt;
  dt = __builtin_fma(r, d1, ms + b5); d2 = d1; d1 = dt;
  dt = step(b4, d1, d2); d2 = d1; d1 = dt;
  dt = step(b3, d1, d2); d2 = d1; d1 = dt;
  dt = step(b2, d1, d2); d2 = d1; d1 = dt;
  dt = step(b1, d1, d2); d2 = d1; d1 = dt;
  const cplx bs = {__builtin_fma(zh.re, d1, __builtin_fma(ms, d2, b0)), zh.im * d1};
  return cdiv(as, bs);
}

// deterministic workgroup sum (fixed order: lanes by butterfly, then waves in index order)
__device__ __forceinline__ double block_sum(double v, double* scratch /*[nwaves]*/, int tid, int nthreads) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  __syncthreads();
  if ((tid & (WAVE - 1)) == 0) scratch[tid / WAVE] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nthreads / WAVE; ++w) s += scratch[w];
  return s;
}

}  // namespace mwrt
