// mwrt_oe.hip -- one optimal-estimation (1D-Var) step per profile on the device (include/mwrt.h mwrt_oe_step_device,
// DESIGN 4.6):   x+ = xa + Sa K^T (K Sa K^T + Se)^-1 [ y - F(x) + K (x - xa) ]     (Rodgers 2000, eq. 5.10, m-form)
//
// One workgroup of 256 threads per profile, everything of the profile's m x m system in LDS:
//   1  x - xa into LDS; a non-finite state ends the profile (status 0)
//   2  one wave per observation row: finiteness of the row (y, F, K, Se) and d = y - F + K (x - xa)
//   3  G = K Sa K^T in column panels of Sa: W_p = K Sa[:, panel] as register tiles (a thread owns rows ti + 32 r and
//      four columns), K and Sa staged through LDS 16 contraction indices at a time with the next chunk's loads in
//      flight; then G += W_p K[:, panel]^T in 4 x 4 tiles of the packed lower triangle.  W is never stored.
//   4  + Se; a dropped row becomes a row of the identity; Cholesky in place (right-looking, two barriers per column)
//   5  wave 0 solves L z = d and L^T u = z with the vectors in registers (no barrier): chi2 = z.z
//   6  v = K^T u, x+ = xa + Sa v: two matrix-vector products
//   7  only when dfs or post_var is asked for: L^-1 in place, dfs = m_used - tr(G^-1 Se),
//      post_var = diag Sa - column sums of squares of L^-1 W_p (the panels are formed again)
// Every sum has a fixed order and nothing is shared between workgroups, so a profile's outputs depend on neither its
// batch-mates nor nprof.  Plain fp64 FMAs; no MFMA variant has been built (DESIGN 4.6 says what was measured).
#include "mwrt_oe_blocks.hip.h"

#include <math.h>

namespace mwrt {
namespace oe {

namespace {

template <int MR>
__global__ void __launch_bounds__(THREADS)
k_oe_step(const OeArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  const int m = A.m, n = A.n;
  const LdsPlan P = lds_plan(m, n);
  const int mp = P.mp, kpitch = P.kpitch;
  double* G = smem + P.g;
  double* Wt = smem + P.region;
  double* vbuf = smem + P.region;          // x - xa, later v = K^T u: the panels' buffers are idle then
  double* Ks = smem + P.ks;
  double* Ss = smem + P.ss;
  double* dvec = smem + P.d;
  double* uvec = smem + P.u;
  double* sed = smem + P.sed;
  double* red = smem + P.red;
  int* keep = reinterpret_cast<int*>(smem + P.keep);
  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  double* xnew = A.x_new + (size_t)prof * n;
  double* pvar = A.post_var ? A.post_var + (size_t)prof * n : nullptr;
  // a profile that ends early: x_new and post_var NaN, chi2 and dfs NaN
  auto give_up = [&](uint8_t status, int nobs) {
    for (int k = tid; k < n; k += THREADS) { xnew[k] = quiet_nan(); if (pvar) pvar[k] = quiet_nan(); }
    if (tid == 0) {
      A.status[prof] = status;
      if (A.chi2) A.chi2[prof] = quiet_nan();
      if (A.dfs) A.dfs[prof] = quiet_nan();
      if (A.nobs) A.nobs[prof] = nobs;
    }
  };

  // ---- 1: the state ----
  if (state_bad<true>(xp, xap, n, vbuf, tid)) return give_up(0, 0);

  // ---- 2: rows ----
  for (int i = wave; i < mp; i += THREADS / 64) {
    const Row r = row_rule<true>(A, prof, i, vbuf, lane);
    if (lane == 0) {
      keep[i] = r.keep ? 1 : 0;
      dvec[i] = r.keep ? r.dy + r.kdx : 0.0;
      sed[i] = r.keep ? r.sii : 0.0;
    }
  }
  __syncthreads();
  const int m_used = rows_kept(keep, m);
  if (m_used == 0) {                       // nothing observed: the prior
    for (int k = tid; k < n; k += THREADS) { xnew[k] = xap[k]; if (pvar) pvar[k] = A.sa[(size_t)k * n + k]; }
    if (tid == 0) {
      A.status[prof] = 3;
      if (A.chi2) A.chi2[prof] = 0.0;
      if (A.dfs) A.dfs[prof] = 0.0;
      if (A.nobs) A.nobs[prof] = 0;
    }
    return;
  }

  // ---- 3: G = K Sa K^T ----
  form_G<MR>(A, prof, keep, G, Wt, Ks, Ss, kpitch);

  // ---- 4: + Se, dropped rows, Cholesky ----
  add_se_and_identity_rows(A, keep, sed, G, 1.0, tid);
  if (!cholesky_packed(G, m, tid)) return give_up(2, m_used);

  // ---- 5: the two triangular solves, in wave 0's registers ----
  if (wave == 0) {
    const double chi2 = solve_llt(G, dvec, uvec, m, lane);
    if (lane == 0 && A.chi2) A.chi2[prof] = chi2;
  }
  __syncthreads();

  // ---- 6: v = K^T u, x+ = xa + Sa v ----
  kt_u(A, prof, keep, uvec, vbuf, tid);
  for (int j = tid; j < n; j += THREADS) xnew[j] = xap[j] + sa_times(A.sa, n, j, vbuf);
  if (tid == 0) {
    A.status[prof] = 1;
    if (A.nobs) A.nobs[prof] = m_used;
  }
  if (!A.dfs && !pvar) return;
  __syncthreads();

  // ---- 7: diagnostics from X = L^-1 ----
  invert_lower(G, m, tid);
  if (A.dfs) {                                             // tr(G^-1 Se) = sum_k (X Se X^T)_kk over the rows kept
    double part = 0.0;
    for (int r = tid >> 4; r < m; r += THREADS / 16)
      for (int c = tid & 15; c <= r; c += 16) {
        const double xrc = G[tri(r, c)];
        if (!keep[c]) continue;
        if (A.se_full) {
          double t = 0.0;                                  // (X Se)_rc = sum_{i <= r} X_ri Se_ic
          for (int i = 0; i <= r; ++i)
            if (keep[i]) t = fma(G[tri(r, i)], A.se[(size_t)i * m + c], t);
          part = fma(t, xrc, part);
        } else {
          part = fma(xrc * xrc, sed[c], part);
        }
      }
    const double trace = block_sum(part, red, tid);
    if (tid == 0) A.dfs[prof] = (double)m_used - trace;
  }
  if (pvar) {
    const int ti = tid >> 3, tj = tid & 7;
    double* colsum = Ks;                                   // [ROW_TILE][PANEL]: Ks and Ss are contiguous and hold >= 1040 doubles
    for (int j0 = 0; j0 < n; j0 += PANEL) {
      form_panel<MR>(A, prof, keep, j0, Wt, Ks, Ss, kpitch, tid);
      // the tile Z = X W_p and its column sums of squares, written out here and in char_gain (mwrt_oe_char.hip says why)
      double z[MR][4];
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[r][c] = 0.0;
      for (int k = 0; k < m; ++k) {                        // Z = X W_p, X lower triangular
        double xr[MR], w[4];
#pragma unroll
        for (int r = 0; r < MR; ++r) {
          const int i = ti + ROW_TILE * r;
          xr[r] = (i < m && k <= i) ? G[tri(i, k)] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = Wt[(tj * 4 + c) * kpitch + k];
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) z[r][c] = fma(xr[r], w[c], z[r][c]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < MR; ++r) s = fma(z[r][c], z[r][c], s);
        colsum[ti * PANEL + tj * 4 + c] = s;
      }
      __syncthreads();
      if (tid < PANEL && j0 + tid < n) {
        const int j = j0 + tid;
        pvar[j] = A.sa[(size_t)j * n + j] - column_total(colsum, tid);
      }
      __syncthreads();
    }
  }
}

template <int MR>
hipError_t launch_mr(const OeArgs& a, int64_t nprof, size_t lds, hipStream_t st) {
  // 151 KiB of LDS at m = 140, n = 4096: inside a workgroup's 160 KiB
  return launch_raised<k_oe_step<MR>>(a, nprof, lds, st);
}

}  // namespace

hipError_t launch_oe_step(const OeArgs& a, int64_t nprof, hipStream_t st) {
  const size_t lds = lds_plan(a.m, a.n).total_bytes;
  switch ((a.m + ROW_TILE - 1) / ROW_TILE) {
    case 1: return launch_mr<1>(a, nprof, lds, st);
    case 2: return launch_mr<2>(a, nprof, lds, st);
    case 3: return launch_mr<3>(a, nprof, lds, st);
    case 4: return launch_mr<4>(a, nprof, lds, st);
    case 5: return launch_mr<5>(a, nprof, lds, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace oe
}  // namespace mwrt
