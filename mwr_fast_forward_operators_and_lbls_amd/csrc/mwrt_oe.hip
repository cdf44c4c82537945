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
#include <atomic>

namespace mwrt {
namespace oe {

namespace {

template <int MR>
__global__ void __launch_bounds__(THREADS)
k_oe_step(const OeArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  const int m = A.m, n = A.n, nlev = A.nlev;
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
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  double* xnew = A.x_new + (size_t)prof * n;
  double* pvar = A.post_var ? A.post_var + (size_t)prof * n : nullptr;

  // ---- 1: the state ----
  int bad = 0;
  for (int k = tid; k < n; k += THREADS) {
    const double xv = xp[k], xav = xap[k];
    bad |= !finite_f64(xv) || !finite_f64(xav);
    vbuf[k] = xv - xav;
  }
  if (__syncthreads_or(bad)) {
    for (int k = tid; k < n; k += THREADS) { xnew[k] = qnan; if (pvar) pvar[k] = qnan; }
    if (tid == 0) {
      A.status[prof] = 0;
      if (A.chi2) A.chi2[prof] = qnan;
      if (A.dfs) A.dfs[prof] = qnan;
      if (A.nobs) A.nobs[prof] = 0;
    }
    return;
  }

  // ---- 2: rows ----
  for (int i = wave; i < mp; i += THREADS / 64) {
    bool ok = false;
    double acc = 0.0, dy = 0.0, sii = 0.0;
    if (i < m) {
      const double yv = A.y[(size_t)prof * m + i], fv = A.fx[(size_t)prof * m + i];
      ok = finite_f64(yv) && finite_f64(fv);
      dy = yv - fv;
      if (A.se_full) {
        for (int c = lane; c < m; c += 64) ok = ok && finite_f64(A.se[(size_t)i * m + c]);
        sii = A.se[(size_t)i * m + i];
      } else {
        sii = A.se[i];
        ok = ok && finite_f64(sii);
      }
      for (int b = 0; b < A.nblk; ++b) {
        const double* row = kblock(A, b, prof) + (size_t)i * nlev;
        const double* dx = vbuf + b * nlev;
        for (int l = lane; l < nlev; l += 64) {
          const double kv = row[l];
          ok = ok && finite_f64(kv);
          acc = fma(kv, dx[l], acc);
        }
      }
      ok = __all(ok);
      acc = wave_sum(acc);
    }
    if (lane == 0) {
      keep[i] = ok ? 1 : 0;
      dvec[i] = ok ? dy + acc : 0.0;
      sed[i] = ok ? sii : 0.0;
    }
  }
  __syncthreads();
  int m_used = 0;
  for (int i = 0; i < m; ++i) m_used += keep[i];
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
  const int ng = m * (m + 1) / 2;
  for (int e = tid; e < ng; e += THREADS) G[e] = 0.0;
  __syncthreads();
  const int nb = (m + 3) / 4, ntiles = nb * (nb + 1) / 2;
  for (int j0 = 0; j0 < n; j0 += PANEL) {
    form_panel<MR>(A, prof, keep, j0, Wt, Ks, Ss, kpitch, tid);
    for (int h = 0; h < PANEL / KCHUNK; ++h) {
      Chunk<MR, false> ch;
      ch.fetch(A, prof, keep, j0 + KCHUNK * h, 0, tid);      // K[:, panel half]; columns beyond n are 0
      ch.store(Ks, Ss, kpitch, tid);
      __syncthreads();
      for (int tile = tid; tile < ntiles; tile += THREADS) {
        int bi = (int)((sqrtf(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);
        while (bi * (bi + 1) / 2 > tile) --bi;
        while ((bi + 1) * (bi + 2) / 2 <= tile) ++bi;
        const int bj = tile - bi * (bi + 1) / 2;
        double t[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) t[a][c] = 0.0;
#pragma unroll 4
        for (int jj = 0; jj < KCHUNK; ++jj) {
          double w[4], q[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) w[a] = Wt[(KCHUNK * h + jj) * kpitch + 4 * bi + a];
#pragma unroll
          for (int c = 0; c < 4; ++c) q[c] = Ks[jj * kpitch + 4 * bj + c];
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) t[a][c] = fma(w[a], q[c], t[a][c]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = 4 * bi + a, j = 4 * bj + c;
            if (i < m && j <= i) G[tri(i, j)] += t[a][c];
          }
      }
      __syncthreads();
    }
  }

  // ---- 4: + Se, dropped rows, Cholesky ----
  if (A.se_full) {
    for (int i = tid >> 4; i < m; i += THREADS / 16)
      for (int c = tid & 15; c < i; c += 16)
        if (keep[i] && keep[c]) G[tri(i, c)] += A.se[(size_t)i * m + c];
  }
  for (int i = tid; i < m; i += THREADS) {
    if (keep[i]) G[tri(i, i)] += sed[i];
    else G[tri(i, i)] = 1.0;
  }
  __syncthreads();
  bool notpd = false;
  for (int j = 0; j < m; ++j) {
    const double piv = G[tri(j, j)];
    if (!(piv > 0.0)) { notpd = true; break; }             // the same value in every thread: a uniform exit
    const double ljj = sqrt(piv);
    for (int i = j + 1 + tid; i < m; i += THREADS) G[tri(i, j)] /= ljj;
    __syncthreads();
    for (int i = j + 1 + (tid >> 4); i < m; i += THREADS / 16) {
      const double lij = G[tri(i, j)];
      for (int c = j + 1 + (tid & 15); c <= i; c += 16) G[tri(i, c)] = fma(-lij, G[tri(c, j)], G[tri(i, c)]);
    }
    if (tid == 0) G[tri(j, j)] = ljj;                      // nobody reads the pivot in this phase
    __syncthreads();
  }
  if (notpd) {
    for (int k = tid; k < n; k += THREADS) { xnew[k] = qnan; if (pvar) pvar[k] = qnan; }
    if (tid == 0) {
      A.status[prof] = 2;
      if (A.chi2) A.chi2[prof] = qnan;
      if (A.dfs) A.dfs[prof] = qnan;
      if (A.nobs) A.nobs[prof] = m_used;
    }
    return;
  }

  // ---- 5: the two triangular solves, in wave 0's registers ----
  if (wave == 0) {
    double v0 = lane < m ? dvec[lane] : 0.0;
    double v1 = lane + 64 < m ? dvec[lane + 64] : 0.0;
    double v2 = lane + 128 < m ? dvec[lane + 128] : 0.0;
    for (int j = 0; j < m; ++j) {                          // L z = d
      const int s = j >> 6, src = j & 63;
      const double zj = __shfl(s == 0 ? v0 : s == 1 ? v1 : v2, src) / G[tri(j, j)];
      if (lane == src) { if (s == 0) v0 = zj; else if (s == 1) v1 = zj; else v2 = zj; }
      int i = lane;
      if (i > j && i < m) v0 = fma(-G[tri(i, j)], zj, v0);
      i = lane + 64;
      if (i > j && i < m) v1 = fma(-G[tri(i, j)], zj, v1);
      i = lane + 128;
      if (i > j && i < m) v2 = fma(-G[tri(i, j)], zj, v2);
    }
    const double chi2 = wave_sum(fma(v0, v0, fma(v1, v1, v2 * v2)));
    if (lane == 0 && A.chi2) A.chi2[prof] = chi2;
    for (int j = m - 1; j >= 0; --j) {                     // L^T u = z
      const int s = j >> 6, src = j & 63;
      const double uj = __shfl(s == 0 ? v0 : s == 1 ? v1 : v2, src) / G[tri(j, j)];
      if (lane == src) { if (s == 0) v0 = uj; else if (s == 1) v1 = uj; else v2 = uj; }
      int i = lane;
      if (i < j) v0 = fma(-G[tri(j, i)], uj, v0);
      i = lane + 64;
      if (i < j) v1 = fma(-G[tri(j, i)], uj, v1);
      i = lane + 128;
      if (i < j) v2 = fma(-G[tri(j, i)], uj, v2);
    }
    if (lane < m) uvec[lane] = v0;
    if (lane + 64 < m) uvec[lane + 64] = v1;
    if (lane + 128 < m) uvec[lane + 128] = v2;
  }
  __syncthreads();

  // ---- 6: v = K^T u, x+ = xa + Sa v ----
  for (int k = tid; k < n; k += THREADS) {
    const int b = k / nlev;
    const double* col = kblock(A, b, prof) + (k - b * nlev);
    double acc = 0.0;
#pragma unroll 14
    for (int i = 0; i < m; ++i) {                          // loads first, the select after: a dropped row may hold NaN
      const double kv = col[(size_t)i * nlev];
      acc = fma(keep[i] ? kv : 0.0, uvec[i], acc);
    }
    vbuf[k] = acc;
  }
  __syncthreads();
  for (int j = tid; j < n; j += THREADS) {
    const double* col = A.sa + j;                          // Sa is symmetric: column j read as row j, coalesced over j
    double acc = 0.0;
#pragma unroll 16
    for (int k = 0; k < n; ++k) acc = fma(col[(size_t)k * n], vbuf[k], acc);
    xnew[j] = xap[j] + acc;
  }
  if (tid == 0) {
    A.status[prof] = 1;
    if (A.nobs) A.nobs[prof] = m_used;
  }
  if (!A.dfs && !pvar) return;
  __syncthreads();

  // ---- 7: diagnostics from X = L^-1 (in place, Gauss-Jordan on the rows) ----
  for (int k = 0; k < m; ++k) {
    const double xkk = 1.0 / G[tri(k, k)];
    for (int j = tid; j < k; j += THREADS) G[tri(k, j)] *= xkk;
    __syncthreads();
    for (int i = k + 1 + (tid >> 4); i < m; i += THREADS / 16) {
      const double lik = G[tri(i, k)];
      for (int j = tid & 15; j < k; j += 16) G[tri(i, j)] = fma(-lik, G[tri(k, j)], G[tri(i, j)]);
    }
    __syncthreads();
    for (int i = k + 1 + tid; i < m; i += THREADS) G[tri(i, k)] *= -xkk;
    if (tid == 0) G[tri(k, k)] = xkk;
    __syncthreads();
  }
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
        double s = 0.0;
        for (int r = 0; r < ROW_TILE; ++r) s += colsum[r * PANEL + tid];
        const int j = j0 + tid;
        pvar[j] = A.sa[(size_t)j * n + j] - s;
      }
      __syncthreads();
    }
  }
}

template <int MR>
hipError_t launch_mr(const OeArgs& a, int64_t nprof, size_t lds, hipStream_t st) {
  // beyond the default dynamic LDS limit from m = 65 on (151 KiB at m = 140, n = 4096: inside a workgroup's 160 KiB).  The
  // limit of an instantiation is raised when a launch first needs more than it had on that device, so a repeat call of
  // the same (or a smaller) size makes no attribute call -- nothing but the launch, which a capturing stream accepts
  if (lds > 64 * 1024) {
    constexpr int MAX_DEV = 64;
    static std::atomic<size_t> raised[MAX_DEV];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEV || raised[dev].load(std::memory_order_acquire) < lds) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_oe_step<MR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < MAX_DEV) raised[dev].store(lds, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(k_oe_step<MR>, dim3((unsigned)nprof), dim3(THREADS), lds, st, a);
  return hipGetLastError();
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
