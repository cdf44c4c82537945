// mwrt_tl_dev.hip.h -- device helpers the tangent-linear units share (csrc/mwrt_tl.hip: the K-matrix; csrc/mwrt_par.hip:
// the spectroscopic-parameter Jacobian): the two-direction tangent type of k_absorb_tl, the Hui rational with its
// derivative, the layer rule with its partials and the deterministic workgroup scans of the adjoint RTE.  Everything is
// __forceinline__: a unit that includes this header gets no symbol from it.
#pragma once
#include "mwrt_math.hip.h"
#include "mwrt_layer.hip.h"           // LOGMEAN_SMALL_S

namespace mwrt {

// ---------------------------------------------------------------------------------------------
// Forward-mode tangents in two directions: value, d/dT at fixed e, d/de at fixed T
// ---------------------------------------------------------------------------------------------
struct dd { double v, t, e; };
__device__ __forceinline__ dd operator+(dd a, dd b) { return {a.v + b.v, a.t + b.t, a.e + b.e}; }
__device__ __forceinline__ dd operator-(dd a, dd b) { return {a.v - b.v, a.t - b.t, a.e - b.e}; }
__device__ __forceinline__ dd operator*(dd a, dd b) {
  return {a.v * b.v, __builtin_fma(a.t, b.v, a.v * b.t), __builtin_fma(a.e, b.v, a.v * b.e)};
}
__device__ __forceinline__ dd operator*(double s, dd a) { return {s * a.v, s * a.t, s * a.e}; }
__device__ __forceinline__ dd operator+(dd a, double s) { return {a.v + s, a.t, a.e}; }
__device__ __forceinline__ dd operator+(double s, dd a) { return {a.v + s, a.t, a.e}; }
__device__ __forceinline__ dd ddiv(dd a, dd b) {
  const double r = fdiv(1.0, b.v), q = a.v * r;
  return {q, (a.t - q * b.t) * r, (a.e - q * b.e) * r};
}
__device__ __forceinline__ dd dexp(dd a) { const double v = fexp(a.v); return {v, v * a.t, v * a.e}; }

__device__ __forceinline__ cplx cscale(cplx a, double s) { return {a.re * s, a.im * s}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx caddc(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ double re_mul(cplx a, cplx b) { return __builtin_fma(a.re, b.re, -a.im * b.im); }

// Hui, Armstrong & Wray's rational w ~ P(zh) / Q(zh) (dcerror_upper) and its derivative dw/dzh, zh = |y| - i x = the
// principal square root the speed-dependent shape feeds it.  The tangent is that of the rational the values use (so
// the K-matrix is the exact derivative of the computed absorption); the true function's w' = -2 z w + 2 i / sqrt(pi)
// differs from it by the rational's own ~1e-6 error.
__device__ __forceinline__ void hui_w_dw(cplx zh, cplx& w, cplx& dw) {
  const double a[7] = {122.607931777104326, 214.382388694706425, 181.928533092181549, 93.155580458138441,
                       30.180142196210589, 5.912626209773153, 0.564189583562615};
  const double b[7] = {122.607931773875350, 352.730625110963558, 457.334478783897737, 348.703917719495792,
                       170.354001821091472, 53.992906912940207, 10.479857114260399};
  cplx p = {a[6], 0.0}, dp = {0.0, 0.0};
#pragma unroll
  for (int k = 5; k >= 0; --k) { dp = caddc(cmul(dp, zh), p); p = cadd(cmul(p, zh), a[k]); }
  cplx q = {1.0, 0.0}, dq = {0.0, 0.0};
#pragma unroll
  for (int k = 6; k >= 0; --k) { dq = caddc(cmul(dq, zh), q); q = cadd(cmul(q, zh), b[k]); }
  const cplx iq = crecip(q);
  w = cmul(p, iq);
  dw = cmul(csub(dp, cmul(w, dq)), iq);
}

// log-mean layer value and its two partial derivatives, branch for branch as layer_value<ZEROFLG>.  ZEROFLG = false
// (cloud liquid and ice): a layer with a zero end has the value 0 and the partials (0, 0) -- the derivative of the branch
// taken; the log-mean's own one-sided slope at a zero end is infinite
template <bool ZEROFLG = true>
__device__ __forceinline__ double layer_value_tl(double x1, double x0, double& d1, double& d0, bool& neg) {
  if (x0 < 0.0 || x1 < 0.0) { neg = true; d1 = d0 = 0.0; return 0.0; }
  const double d = x1 - x0;
  if (fabs(d) < 1e-09) { d1 = 1.0; d0 = 0.0; return x1; }
  if (x0 == 0.0 || x1 == 0.0) { d1 = d0 = ZEROFLG ? 0.5 : 0.0; return ZEROFLG ? 0.5 * (x1 + x0) : 0.0; }
  const double sm = x1 + x0, ism = fdiv(1.0, sm), s = d * ism;
  if (fabs(s) <= LOGMEAN_SMALL_S) {
    // L = sm/2 q(z), q = s/atanh(s), z = s^2:  dL/dx1 = q/2 + 2 s q'(z) x0/sm,  dL/dx0 = q/2 - 2 s q'(z) x1/sm
    const double z = s * s;
    const double c[10] = {-3.3333333333333333333e-01, -8.8888888888888888889e-02, -4.6560846560846560847e-02,
                          -3.0194003527336860670e-02, -2.1796804019026241248e-02, -1.6787551856334925118e-02,
                          -1.3502765051265933100e-02, -1.1203745637718733130e-02, -9.5160731945278989134e-03,
                          -8.2312065673505011548e-03};
    double q = 0.0, qp = 0.0;
#pragma unroll
    for (int k = 9; k >= 0; --k) { qp = __builtin_fma(qp, z, (k + 1) * c[k]); q = (q + c[k]) * z; }
    q += 1.0;
    const double u = 2.0 * s * qp * ism;
    d1 = __builtin_fma(u, x0, 0.5 * q);
    d0 = __builtin_fma(-u, x1, 0.5 * q);
    return 0.5 * sm * q;
  }
  const double ln = flog(fdiv(x1, x0)), iln = fdiv(1.0, ln), L = d * iln;
  d1 = (1.0 - fdiv(L, x1)) * iln;
  d0 = (fdiv(L, x0) - 1.0) * iln;
  return L;
}

// inclusive prefix sum over the workgroup (lanes by shuffles, then the waves in index order: deterministic)
__device__ __forceinline__ double block_scan(double v, double* wsum, int tid, int nwaves, double& total) {
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const double u = __shfl_up(v, o, WAVE);
    if (lane >= o) v += u;
  }
  __syncthreads();
  if (lane == WAVE - 1) wsum[wave] = v;
  __syncthreads();
  double off = 0.0, tot = 0.0;
  for (int w = 0; w < nwaves; ++w) {
    const double x = wsum[w];
    off += (w < wave) ? x : 0.0;
    tot += x;
  }
  total = tot;
  return v + off;
}

// exclusive suffix sum over the workgroup: the sum of v over the lanes above tid (lanes by shuffles, then the waves
// above in a fixed order: deterministic).  Summed from the top down, never as a total minus a prefix: where the terms
// above are tiny (levels an opaque path hides) the result keeps its relative accuracy.
__device__ __forceinline__ double block_suffix_excl(double v, double* wsum, int tid, int nwaves) {
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const double u = __shfl_down(v, o, WAVE);
    if (lane + o < WAVE) v += u;
  }
  __syncthreads();                     // (wsum may still be read by a previous scan)
  if (lane == 0) wsum[wave] = v;       // the wave's total
  __syncthreads();
  const double nxt = __shfl_down(v, 1, WAVE);
  double off = 0.0;
  for (int w = nwaves - 1; w > wave; --w) off += wsum[w];
  return ((lane + 1 < WAVE) ? nxt : 0.0) + off;
}

}  // namespace mwrt
