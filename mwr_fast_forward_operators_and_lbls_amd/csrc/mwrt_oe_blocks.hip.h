// mwrt_oe_blocks.hip.h -- the device building blocks the optimal-estimation kernel units share (csrc/mwrt_oe.hip,
// csrc/mwrt_oe_lm.hip and csrc/mwrt_oe_char.hip, DESIGN 4.6 with its table of blocks): finiteness, the packed-triangle
// index, the K-block row base, the wave and block sums, the register chunk of K and Sa, the panel W_p = K Sa[:, panel], the
// factorisation and the solves, the numbered steps of k_oe_step that its split and its characterisation repeat, and the
// launcher that raises a kernel's LDS limit.  A block keeps the order of every sum, the thread-to-element mapping and the
// barriers it had when it was written out in the kernels; its comment says whether it ends behind a barrier.  Device units
// only: the host unit never includes this file.  Everything is force-inlined and sits in an unnamed namespace, so each unit
// gets its own copy.
#pragma once
#include "mwrt_oe.hip.h"

#include <math.h>
#include <atomic>

namespace mwrt {
namespace oe {

namespace {

__device__ __forceinline__ bool finite_f64(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, j <= i

// row base of K block b of this profile: entry [i][l] is at base[i * nlev + l]
__device__ __forceinline__ const double* kblock(const OeArgs& A, int b, int64_t prof) {
  const double* p = b == 0 ? A.k0 : b == 1 ? A.k1 : b == 2 ? A.k2 : A.k3;
  return p + (size_t)prof * A.m * A.nlev;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum of one value per thread in a fixed tree; every thread gets the result.  `red` is left free for the next use.
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// one chunk of KCHUNK contraction indices in registers: K[:, k0 .. k0 + 16) (rows li + 16 r) and, with SA,
// Sa[k0 .. k0 + 16)[j0 .. j0 + 32)
template <int MR, bool SA>
struct Chunk {
  double k[2 * MR];
  double s[2];
  __device__ __forceinline__ void fetch(const OeArgs& A, int64_t prof, const int* keep, int k0, int j0, int tid) {
    const int lkk = tid & (KCHUNK - 1), li = tid >> 4;
    const int kk = k0 + lkk;
    const bool kin = kk < A.n;
    const int b = kin ? kk / A.nlev : 0;
    const double* base = kblock(A, b, prof) + (kin ? kk - b * A.nlev : 0);
#pragma unroll
    for (int r = 0; r < 2 * MR; ++r) {
      const int i = li + 16 * r;
      const bool live = kin && i < A.m && keep[i] != 0;
      k[r] = live ? base[(size_t)i * A.nlev] : 0.0;
    }
    if (SA) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int e = tid + THREADS * q;
        const int kr = k0 + (e >> 5), jc = j0 + (e & (PANEL - 1));
        s[q] = (kr < A.n && jc < A.n) ? A.sa[(size_t)kr * A.n + jc] : 0.0;
      }
    }
  }
  __device__ __forceinline__ void store(double* Ks, double* Ss, int kpitch, int tid) const {
    const int lkk = tid & (KCHUNK - 1), li = tid >> 4;
#pragma unroll
    for (int r = 0; r < 2 * MR; ++r) Ks[lkk * kpitch + li + 16 * r] = k[r];
    if (SA) {
#pragma unroll
      for (int q = 0; q < 2; ++q) Ss[tid + THREADS * q] = s[q];
    }
  }
};

// W_p = K Sa[:, j0 .. j0 + 32) into Wt [PANEL][kpitch] (transposed: Wt[jj][i]).  Ends behind a barrier.
template <int MR>
__device__ __forceinline__ void form_panel(const OeArgs& A, int64_t prof, const int* keep, int j0, double* Wt, double* Ks,
                                           double* Ss, int kpitch, int tid) {
  const int ti = tid >> 3, tj = tid & 7;
  double acc[MR][4];
#pragma unroll
  for (int r = 0; r < MR; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  Chunk<MR, true> ch;
  ch.fetch(A, prof, keep, 0, j0, tid);
  for (int k0 = 0; k0 < A.n; k0 += KCHUNK) {
    ch.store(Ks, Ss, kpitch, tid);
    __syncthreads();
    if (k0 + KCHUNK < A.n) ch.fetch(A, prof, keep, k0 + KCHUNK, j0, tid);   // in flight while this chunk is contracted
#pragma unroll
    for (int kk = 0; kk < KCHUNK; ++kk) {
      double a[MR], s[4];
#pragma unroll
      for (int r = 0; r < MR; ++r) a[r] = Ks[kk * kpitch + ti + ROW_TILE * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = Ss[kk * PANEL + tj * 4 + c];
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], s[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < MR; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) Wt[(tj * 4 + c) * kpitch + ti + ROW_TILE * r] = acc[r][c];
  __syncthreads();
}

// G += W_p[:, half h] K[:, panel half]^T in 4 x 4 tiles of the packed lower triangle (k_oe_step, step 3)
__device__ __forceinline__ void triangle_update(double* G, const double* Wt, const double* Ks, int kpitch, int h, int m,
                                                int ntiles, int tid) {
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
}

// Cholesky of the packed lower triangle in place (right-looking, two barriers per column).  False, in every thread, when a
// pivot fails pivot > 0.  Ends behind a barrier.
__device__ __forceinline__ bool cholesky_packed(double* G, int m, int tid) {
  for (int j = 0; j < m; ++j) {
    const double piv = G[tri(j, j)];
    if (!(piv > 0.0)) return false;                        // the same value in every thread: a uniform exit
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
  return true;
}

// One wave, the vector in its registers (entry i in lane i & 63, register i >> 6; m <= 192): L z = d in place.
__device__ __forceinline__ void solve_lower(const double* G, int m, int lane, double& v0, double& v1, double& v2) {
  for (int j = 0; j < m; ++j) {
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
}
// ... and L^T u = z in place
__device__ __forceinline__ void solve_upper(const double* G, int m, int lane, double& v0, double& v1, double& v2) {
  for (int j = m - 1; j >= 0; --j) {
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
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double plus_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// X = L^-1 in place, Gauss-Jordan on the rows (k_oe_step, step 7)
__device__ __forceinline__ void invert_lower(double* G, int m, int tid) {
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
}

// ---- the steps of k_oe_step that its split and its characterisation share (the table of blocks) ----

// Step 1, the state: the thread's own finding, non-zero when an entry of x or xa it looked at is not finite.  With DX,
// x - xa goes to dx[0 .. n).  No barrier: a kernel that has findings of its own (k_lm_solve, k_lm_cost) ors them in and
// makes the verdict uniform with one __syncthreads_or, which also publishes dx.
template <bool DX>
__device__ __forceinline__ int state_scan(const double* xp, const double* xap, int n, double* dx, int tid) {
  int bad = 0;
  for (int k = tid; k < n; k += THREADS) {
    const double xv = xp[k], xav = xap[k];
    bad |= !finite_f64(xv) || !finite_f64(xav);
    if (DX) dx[k] = xv - xav;
  }
  return bad;
}
// ... and the block-uniform verdict.  Ends behind its one barrier.
template <bool DX>
__device__ __forceinline__ bool state_bad(const double* xp, const double* xap, int n, double* dx, int tid) {
  return __syncthreads_or(state_scan<DX>(xp, xap, n, dx, tid)) != 0;
}

// Step 2, the row rule, one wave per row: row i is kept when y, F, its K row and its Se entries are finite (i >= m: not
// kept).  Uniform over the wave.  With KDX the same pass over the K row sums K (x - xa) in lane order and a wave tree;
// without it the row is read once for the verdict alone.  No barrier.
struct Row {
  bool keep;
  double dy, sii, kdx;                     // y - F, Se_ii and K dx of the row: meaningful when it is kept
};
template <bool KDX>
__device__ __forceinline__ Row row_rule(const OeArgs& A, int64_t prof, int i, const double* dxv, int lane) {
  Row r{false, 0.0, 0.0, 0.0};
  if (i >= A.m) return r;
  const int m = A.m, nlev = A.nlev;
  const double yv = A.y[(size_t)prof * m + i], fv = A.fx[(size_t)prof * m + i];
  bool ok = finite_f64(yv) && finite_f64(fv);
  r.dy = yv - fv;
  if (A.se_full) {
    for (int c = lane; c < m; c += 64) ok = ok && finite_f64(A.se[(size_t)i * m + c]);
    r.sii = A.se[(size_t)i * m + i];
  } else {
    r.sii = A.se[i];
    ok = ok && finite_f64(r.sii);
  }
  double acc = 0.0;
  for (int b = 0; b < A.nblk; ++b) {
    const double* row = kblock(A, b, prof) + (size_t)i * nlev;
    for (int l = lane; l < nlev; l += 64) {
      const double kv = row[l];
      ok = ok && finite_f64(kv);
      if (KDX) acc = fma(kv, dxv[b * nlev + l], acc);
    }
  }
  r.keep = __all(ok);
  if (KDX) r.kdx = wave_sum(acc);
  return r;
}

// rows kept, the same count in every thread
__device__ __forceinline__ int rows_kept(const int* keep, int m) {
  int m_used = 0;
  for (int i = 0; i < m; ++i) m_used += keep[i];
  return m_used;
}

// Step 3: the packed lower triangle G = K Sa K^T over the rows kept, panel by panel in the order of the columns of Sa; W
// is never stored.  Ends behind a barrier.  It reads the thread index itself: with `tid` handed in, the compiler hoists
// differently and k_oe_step<2> lands above the register count its test pins.
template <int MR>
__device__ __forceinline__ void form_G(const OeArgs& A, int64_t prof, const int* keep, double* G, double* Wt, double* Ks,
                                       double* Ss, int kpitch) {
  const int tid = threadIdx.x, m = A.m, n = A.n;
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
      triangle_update(G, Wt, Ks, kpitch, h, m, ntiles, tid);
      __syncthreads();
    }
  }
}

// Step 4, before the Cholesky: G += og Se on the rows and columns kept (sed: the kept rows' Se_ii), a dropped row becomes
// a row of the identity (its off-diagonal entries are 0 already: form_G reads a dropped row of K as 0).  The step and the
// gain pass og = 1, where fma(1, Se, G) is G + Se.  Ends behind a barrier.
__device__ __forceinline__ void add_se_and_identity_rows(const OeArgs& A, const int* keep, const double* sed, double* G,
                                                         double og, int tid) {
  const int m = A.m;
  if (A.se_full) {
    for (int i = tid >> 4; i < m; i += THREADS / 16)
      for (int c = tid & 15; c < i; c += 16)
        if (keep[i] && keep[c]) G[tri(i, c)] = fma(og, A.se[(size_t)i * m + c], G[tri(i, c)]);
  }
  for (int i = tid; i < m; i += THREADS) {
    if (keep[i]) G[tri(i, i)] = fma(og, sed[i], G[tri(i, i)]);
    else G[tri(i, i)] = 1.0;
  }
  __syncthreads();
}

// Step 5, wave 0 alone, no barrier: L z = d and L^T u = z with the vectors in its registers; u is stored, z.z returned.
__device__ __forceinline__ double solve_llt(const double* G, const double* d, double* u, int m, int lane) {
  double v0 = lane < m ? d[lane] : 0.0;
  double v1 = lane + 64 < m ? d[lane + 64] : 0.0;
  double v2 = lane + 128 < m ? d[lane + 128] : 0.0;
  solve_lower(G, m, lane, v0, v1, v2);
  const double chi2 = wave_sum(fma(v0, v0, fma(v1, v1, v2 * v2)));
  solve_upper(G, m, lane, v0, v1, v2);
  if (lane < m) u[lane] = v0;
  if (lane + 64 < m) u[lane + 64] = v1;
  if (lane + 128 < m) u[lane + 128] = v2;
  return chi2;
}

// Step 6, first half: v = K^T u over the rows kept, rows in ascending order, thread k owns v[k].  Ends behind a barrier.
__device__ __forceinline__ void kt_u(const OeArgs& A, int64_t prof, const int* keep, const double* u, double* v, int tid) {
  const int m = A.m, nlev = A.nlev;
  for (int k = tid; k < A.n; k += THREADS) {
    const int b = k / nlev;
    const double* col = kblock(A, b, prof) + (k - b * nlev);
    double acc = 0.0;
#pragma unroll 14
    for (int i = 0; i < m; ++i) {                          // loads first, the select after: a dropped row may hold NaN
      const double kv = col[(size_t)i * nlev];
      acc = fma(keep[i] ? kv : 0.0, u[i], acc);
    }
    v[k] = acc;
  }
  __syncthreads();
}

// (S v)_j for a symmetric S [n][n]: column j read as row j, coalesced over j; k ascending.  No barrier.
__device__ __forceinline__ double sa_times(const double* S, int n, int j, const double* v) {
  const double* col = S + j;
  double acc = 0.0;
#pragma unroll 16
  for (int k = 0; k < n; ++k) acc = fma(col[(size_t)k * n], v[k], acc);
  return acc;
}

// Column j of the panel: the threads' sums of squares in colsum [ROW_TILE][PANEL] added in row order.  The caller has
// placed a barrier after the threads stored them.
__device__ __forceinline__ double column_total(const double* colsum, int j) {
  double s = 0.0;
#pragma unroll 4
  for (int r = 0; r < ROW_TILE; ++r) s += colsum[r * PANEL + j];
  return s;
}

// Launch `kernel`, one workgroup of THREADS per profile.  Beyond the default dynamic LDS limit (64 KiB: from m = 65 on in
// the panel kernels) the kernel's limit is raised when a launch first needs more than it had on that device, so a repeat
// call of the same (or a smaller) size makes no attribute call -- nothing but the launch, which a capturing stream accepts.
template <auto kernel, typename Args>
hipError_t launch_raised(const Args& a, int64_t nprof, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024) {
    constexpr int MAX_DEV = 64;
    static std::atomic<size_t> raised[MAX_DEV];            // one per kernel: `kernel` is a template argument
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEV || raised[dev].load(std::memory_order_acquire) < lds) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < MAX_DEV) raised[dev].store(lds, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)nprof), dim3(THREADS), lds, st, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace oe
}  // namespace mwrt
