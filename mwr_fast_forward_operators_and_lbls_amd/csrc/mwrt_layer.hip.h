// mwrt_layer.hip.h -- the layer rule: log-mean value of two adjacent levels, one layer or four at a time.
#pragma once
#include "mwrt_math.hip.h"

namespace mwrt {

// RTEquation.exponential_integration [EXT]: log-mean ("exponential decay") layer value.
// Branch order is the contract.  Returns NaN-flag through `neg`.
//
// The log-mean itself: with s = (x1 - x0)/(x1 + x0),  ln(x1/x0) = 2 atanh(s), so
//   (x1 - x0)/ln(x1/x0) = (x1 + x0)/2 * s/atanh(s),   s/atanh(s) = 1 - s^2/3 - 4 s^4/45 - ...
// Adjacent levels of a sounding differ by a few percent, so |s| <= LOGMEAN_SMALL_S for a whole wave is
// the usual case (wave vote): one division and a 10-term series instead of a division, a full log
// (frexp, second division, series) and a third division.  It is also better conditioned than the
// quotient form, which loses up to 1e-7 relative when x1 - x0 is just above the 1e-9 switch.
constexpr double LOGMEAN_SMALL_S = 0.1715;      // |s| <= this: inside the interval s_over_atanh was fitted on

// s / atanh(s) = 1 - z/3 - 4 z^2/45 - 44 z^3/945 - ... (z = s^2) = 1 + z g(z), g of degree 6 fitted at the Chebyshev nodes
// of [0, 0.1716^2] (1.1e-18 relative; the Taylor series needs ten terms): the log-mean is (x1 + x0)/2 times this
__device__ __forceinline__ double s_over_atanh(double z) {
  double q = -0.014721548786632996;
  MWRT_FMA_SC(q, z, -0.01673734010479199);
  MWRT_FMA_SC(q, z, -0.02179782053718046);
  MWRT_FMA_SC(q, z, -0.03019399300258251);
  MWRT_FMA_SC(q, z, -0.04656084661263456);
  MWRT_FMA_SC(q, z, -0.08888888888879345);
  MWRT_FMA_SC(q, z, -0.33333333333333337);
  return __builtin_fma(q, z, 1.0);
}

// The same quotient on the next band, |s| <= LOGMEAN_MID_S (adjacent absorptions up to 4 : 1, the coarse top of a
// sounding): a (5,5) rational fit in z = s^2 on Chebyshev nodes of [0, 0.36], 7.7e-17 relative in exact arithmetic.
// Ten FMAs and one division, about half of log_mean_any.
constexpr double LOGMEAN_MID_S = 0.6;
__device__ __forceinline__ double s_over_atanh_mid(double z) {
  double pn = -1.24405457430790653678e-02, qd = -1.87173749238921052448e-03;
  MWRT_FMA_SC(pn, z, 2.32467124128396325363e-01);
  MWRT_FMA_SC(qd, z, 9.09554662683649162425e-02);
  MWRT_FMA_SC(pn, z, -1.25179985749945586930e+00);
  MWRT_FMA_SC(qd, z, -7.29233489586724676923e-01);
  MWRT_FMA_SC(pn, z, 2.79764691392900100515e+00);
  MWRT_FMA_SC(qd, z, 2.07624733687436672750e+00);
  MWRT_FMA_SC(pn, z, -2.76419873116542634427e+00);
  MWRT_FMA_SC(qd, z, -2.43086539783209769889e+00);
  pn = __builtin_fma(pn, z, 1.0);
  qd = __builtin_fma(qd, z, 1.0);
  return fdiv1(pn, qd);
}

// The log-mean for ANY ratio of two positive values with one division for the logarithm and one for the quotient:
//   x1/x0 = 2^e m,  m in [1/sqrt 2, sqrt 2]  (e from the exponent fields, x0' = x0 2^e),
//   s' = (x1 - x0')/(x1 + x0'),  ln(x1/x0) = e ln 2 + 2 s' (atanh(s')/s'),  result = (x1 - x0) / ln(x1/x0).
// ln keeps full RELATIVE accuracy as x1 -> x0 (e = 0, ln = 2 s' (1 + z/3 + ...)), which the quotient of a generic
// log cannot.  ~45 VALU, no branch: what a wave runs when some lane's levels are far apart (the coarse top of a
// sounding shares its wave with finely spaced levels).
__device__ __forceinline__ double log_mean_any(double x1, double x0, double d) {
  int e = __builtin_amdgcn_frexp_exp(x1) - __builtin_amdgcn_frexp_exp(x0);
  double x0s = __builtin_amdgcn_ldexp(x0, e);                      // x1 / x0s in (1/2, 2)
  const bool hi = x1 > 1.41421356237309504880 * x0s;
  const bool lo = x1 * 1.41421356237309504880 < x0s;
  x0s = hi ? x0s + x0s : (lo ? 0.5 * x0s : x0s);
  e = hi ? e + 1 : (lo ? e - 1 : e);
  const double sp = fdiv1(x1 - x0s, x1 + x0s);                     // |s'| <= 0.1716
  const double z = sp * sp;
  const double p = __builtin_fma(two_atanh_tail(z), z, 2.0);      // 2 atanh(s)/s = 2 + 2z/3 + 2z^2/5 + ...
  const double ed = (double)e;
  const double ln = __builtin_fma(ed, 6.93147180369123816490e-01, __builtin_fma(ed, 1.90821492927058770002e-10, sp * p));
  return fdiv1(d, ln);
}

template <bool ZEROFLG = true>
__device__ __forceinline__ double layer_value(double x1, double x0, bool& neg, bool live = true) {
  // live = this lane holds a layer (its result is used): the wave votes ignore the others
  const double d = x1 - x0;
  const double sm = x1 + x0;
  const bool same = fabs(d) < 1e-09;
  // x0 < 0 | x1 < 0 | x0 == 0 | x1 == 0 in one comparison (NaN inputs never reach this point)
  const bool nonpos = !(fmin(x1, x0) > 0.0);
  double r;
  const double s = fdiv1(d, sm);
  // the votes as algebra on comparison masks (each ballot is its v_cmp; combining bools first costs two VALU per vote)
  const wmask m_live = __builtin_amdgcn_ballot_w64(live);
  const wmask m_special = (__builtin_amdgcn_ballot_w64(nonpos) | __builtin_amdgcn_ballot_w64(same)) & m_live;
  const wmask m_plain = m_live & ~m_special;                     // lanes whose log-mean is the generic one
  if ((m_plain & ~__builtin_amdgcn_ballot_w64(fabs(s) <= LOGMEAN_SMALL_S)) == 0ull) {
    KEEP_BRANCH();
    r = (0.5 * sm) * s_over_atanh(s * s);
  } else if ((m_plain & ~__builtin_amdgcn_ballot_w64(fabs(s) <= LOGMEAN_MID_S)) == 0ull) {
    KEEP_BRANCH();
    r = (0.5 * sm) * s_over_atanh_mid(s * s);
  } else {
    KEEP_BRANCH();
    r = log_mean_any(x1, x0, d);
  }
  if (m_special != 0ull) {                                     // rare below the stratosphere: wave-uniform skip (and 12 VGPRs fewer live)
    const bool negative = (x0 < 0.0) | (x1 < 0.0);
    const bool zero = x0 == 0.0 || x1 == 0.0;
    if (negative && live) neg = true;
    r = zero ? (ZEROFLG ? sm * 0.5 : 0.0) : r;                 // zeroflg = True for wet & dry, False for liquid & ice
    r = same ? x1 : r;
    r = negative ? 0.0 : r;
  }
  return r;
}

// Four layer values behind ONE pair of wave votes (the TAU absorption kernels make 32 per lane and chunk).
// x1[k] in, layer value out (in place); x0[k] = the level below.
template <bool ZEROFLG = true>
__device__ __forceinline__ void layer_value4(double (&x1)[4], const double (&x0)[4], bool& neg, bool live) {
  double s[4];
  // votes as algebra on comparison masks (see layer_value)
  const wmask m_live = wballot(live);
  wmask m_special = 0ull, m_notsmall = 0ull, m_notmid = 0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = x1[k] - x0[k];
    s[k] = fdiv1(d, x1[k] + x0[k]);
    const wmask sp = wballot(!(fmin(x1[k], x0[k]) > 0.0)) | wballot(fabs(d) < 1e-09);
    m_special |= sp;
    m_notsmall |= ~(sp | wballot(fabs(s[k]) <= LOGMEAN_SMALL_S));
    m_notmid |= ~(sp | wballot(fabs(s[k]) <= LOGMEAN_MID_S));
  }
  m_special &= m_live;
  double r[4];
  if ((m_live & m_notsmall) == 0ull) {
    KEEP_BRANCH();
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (0.5 * (x1[k] + x0[k])) * s_over_atanh(s[k] * s[k]);
  } else if ((m_live & m_notmid) == 0ull) {
    KEEP_BRANCH();
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (0.5 * (x1[k] + x0[k])) * s_over_atanh_mid(s[k] * s[k]);
  } else {
    KEEP_BRANCH();
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = log_mean_any(x1[k], x0[k], x1[k] - x0[k]);
  }
  if (m_special != 0ull) {
    KEEP_BRANCH();
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const double d = x1[k] - x0[k];
      const bool negative = (x0[k] < 0.0) | (x1[k] < 0.0);
      const bool zero = x0[k] == 0.0 || x1[k] == 0.0;
      if (negative && live) neg = true;
      double q = zero ? (ZEROFLG ? (x1[k] + x0[k]) * 0.5 : 0.0) : r[k];
      q = (fabs(d) < 1e-09) ? x1[k] : q;
      r[k] = negative ? 0.0 : q;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) x1[k] = r[k];
}

}  // namespace mwrt
