// mwrt_oe_lm.hip -- the optimal-estimation step split for Levenberg-Marquardt damping (include/mwrt.h mwrt_oe_lm_*_device
// and mwrt_oe_cost_device).  With dx = x - xa, r = y - F(x) and a damping factor gamma >= 0 per profile,
//     x+ = xa + gamma / (1 + gamma) dx + Sa K^T u,     (K Sa K^T + (1 + gamma) Se) u = r + K dx / (1 + gamma)
// is Rodgers 2000, eq. 5.36 in the m-form; gamma = 0 is the step of csrc/mwrt_oe.hip.  G0 = K Sa K^T, r and K dx depend
// on x alone and are all but 1 % of the step's arithmetic, so they are formed once per accepted state and every trial
// gamma pays for the m x m solve only:
//   k_lm_prepare<MR>  steps 1-3 of k_oe_step (state check, row rule, G0 in panels) -> G0, r, K dx, keep in caller-owned HBM
//   k_lm_solve        G0 + (1 + gamma) Se in LDS, Cholesky, the two triangular solves, v = K^T u, x+; chi2 = d^T G^-1 d
//   k_lm_cost         J = r^T Se^-1 r (over the linearisation's rows) + dx^T Sa^-1 dx at a state
// One workgroup of 256 threads per profile in all three; every sum has a fixed order and nothing is shared between
// workgroups, so a profile's outputs depend on neither its batch-mates nor nprof.  The panel, chunk and sum blocks are
// those of k_oe_step (mwrt_oe_blocks.hip.h); the 4 x 4 triangle update, the Cholesky and the solves are written inline in
// that kernel, so this unit carries its own copies of them as functions.
#include "mwrt_oe_lm.hip.h"
#include "mwrt_oe_blocks.hip.h"

#include <math.h>
#include <atomic>

namespace mwrt {
namespace lm {

namespace {

using oe::OeArgs;
using oe::finite_f64;
using oe::tri;
using oe::kblock;
using oe::wave_sum;
using oe::block_sum;
using oe::KCHUNK;
using oe::PANEL;

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

// ---- the linearisation: G0 = K Sa K^T, r = y - F(x), K (x - xa), the rows kept ----
template <int MR>
__global__ void __launch_bounds__(THREADS)
k_lm_prepare(const LmArgs L) {
  extern __shared__ double smem[];
  const OeArgs& A = L.o;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (L.active && L.active[prof] == 0) return;
  const int m = A.m, n = A.n, nlev = A.nlev;
  const oe::LdsPlan P = oe::lds_plan(m, n);
  const int mp = P.mp, kpitch = P.kpitch;
  double* G = smem + P.g;
  double* Wt = smem + P.region;
  double* vbuf = smem + P.region;          // x - xa: the panels' buffers are idle until step 3
  double* Ks = smem + P.ks;
  double* Ss = smem + P.ss;
  int* keep = reinterpret_cast<int*>(smem + P.keep);

  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  double* rout = L.r + (size_t)prof * m;
  double* kout = L.kdx + (size_t)prof * m;
  uint8_t* keepout = L.keep + (size_t)prof * m;
  const int ng = m * (m + 1) / 2;
  double* g0 = L.g0 + (size_t)prof * ng;

  // ---- 1: the state ----
  int bad = 0;
  for (int k = tid; k < n; k += THREADS) {
    const double xv = xp[k], xav = xap[k];
    bad |= !finite_f64(xv) || !finite_f64(xav);
    vbuf[k] = xv - xav;
  }
  if (__syncthreads_or(bad)) {
    for (int i = tid; i < m; i += THREADS) { rout[i] = quiet_nan(); kout[i] = quiet_nan(); keepout[i] = 0; }
    for (int e = tid; e < ng; e += THREADS) g0[e] = quiet_nan();
    if (tid == 0) L.lin_status[prof] = 0;
    return;
  }

  // ---- 2: rows ----
  for (int i = wave; i < mp; i += THREADS / 64) {
    bool ok = false;
    double acc = 0.0, dy = 0.0;
    if (i < m) {
      const double yv = A.y[(size_t)prof * m + i], fv = A.fx[(size_t)prof * m + i];
      ok = finite_f64(yv) && finite_f64(fv);
      dy = yv - fv;
      if (A.se_full) {
        for (int c = lane; c < m; c += 64) ok = ok && finite_f64(A.se[(size_t)i * m + c]);
      } else {
        ok = ok && finite_f64(A.se[i]);
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
      if (i < m) {
        keepout[i] = ok ? 1 : 0;
        rout[i] = ok ? dy : 0.0;
        kout[i] = ok ? acc : 0.0;
      }
    }
  }
  __syncthreads();
  int m_used = 0;
  for (int i = 0; i < m; ++i) m_used += keep[i];
  if (m_used == 0) {                       // nothing observed: G0 = 0
    for (int e = tid; e < ng; e += THREADS) g0[e] = 0.0;
    if (tid == 0) L.lin_status[prof] = 3;
    return;
  }

  // ---- 3: G0 = K Sa K^T ----
  for (int e = tid; e < ng; e += THREADS) G[e] = 0.0;
  __syncthreads();
  const int nb = (m + 3) / 4, ntiles = nb * (nb + 1) / 2;
  for (int j0 = 0; j0 < n; j0 += PANEL) {
    oe::form_panel<MR>(A, prof, keep, j0, Wt, Ks, Ss, kpitch, tid);
    for (int h = 0; h < PANEL / KCHUNK; ++h) {
      oe::Chunk<MR, false> ch;
      ch.fetch(A, prof, keep, j0 + KCHUNK * h, 0, tid);      // K[:, panel half]; columns beyond n are 0
      ch.store(Ks, Ss, kpitch, tid);
      __syncthreads();
      triangle_update(G, Wt, Ks, kpitch, h, m, ntiles, tid);
      __syncthreads();
    }
  }
  for (int e = tid; e < ng; e += THREADS) g0[e] = G[e];
  if (tid == 0) L.lin_status[prof] = 1;
}

// ---- one damped trial on a linearisation ----
__global__ void __launch_bounds__(THREADS)
k_lm_solve(const LmArgs L) {
  extern __shared__ double smem[];
  const OeArgs& A = L.o;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (L.active && L.active[prof] == 0) return;
  const int m = A.m, n = A.n, nlev = A.nlev;
  const SolvePlan P = solve_plan(m, n);
  double* G = smem + P.g;
  double* dvec = smem + P.d;
  double* uvec = smem + P.u;
  double* vbuf = smem + P.v;
  int* keep = reinterpret_cast<int*>(smem + P.keep);

  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  double* xnew = A.x_new + (size_t)prof * n;
  const double gamma = L.gamma[prof];
  const int lin = L.lin_status[prof];
  const bool gamma_ok = finite_f64(gamma) && gamma >= 0.0;
  const double og = 1.0 + gamma;           // >= 1 when gamma_ok
  const double wdx = gamma / og;           // the weight of x - xa that damping leaves in x+

  int bad = 0;
  for (int k = tid; k < n; k += THREADS) bad |= !finite_f64(xp[k]) || !finite_f64(xap[k]);
  for (int i = tid; i < m; i += THREADS) {
    const int kp = L.keep[(size_t)prof * m + i] != 0;
    keep[i] = kp;
    dvec[i] = kp ? L.r[(size_t)prof * m + i] + L.kdx[(size_t)prof * m + i] / og : 0.0;
  }
  bad = __syncthreads_or(bad);
  int m_used = 0;
  for (int i = 0; i < m; ++i) m_used += keep[i];
  if (bad || lin == 0 || !gamma_ok) {      // the state (now, or when it was linearised) not finite: 0; gamma refused: 2
    const bool state = bad || lin == 0;
    for (int k = tid; k < n; k += THREADS) xnew[k] = quiet_nan();
    if (tid == 0) {
      A.status[prof] = state ? 0 : 2;
      if (A.chi2) A.chi2[prof] = quiet_nan();
      if (A.nobs) A.nobs[prof] = state ? 0 : m_used;
    }
    return;
  }
  if (lin == 3 || m_used == 0) {           // nothing observed: the damped pull towards the prior alone
    for (int k = tid; k < n; k += THREADS) xnew[k] = xap[k] + wdx * (xp[k] - xap[k]);
    if (tid == 0) {
      A.status[prof] = 3;
      if (A.chi2) A.chi2[prof] = 0.0;
      if (A.nobs) A.nobs[prof] = 0;
    }
    return;
  }

  // ---- 4: G0 + (1 + gamma) Se on the rows and columns kept, a dropped row a row of the identity; Cholesky ----
  const double* g0 = L.g0 + (size_t)prof * (m * (m + 1) / 2);
  for (int i = tid >> 4; i < m; i += THREADS / 16)
    for (int c = tid & 15; c <= i; c += 16) {
      double g = c == i ? 1.0 : 0.0;
      if (keep[i] && keep[c]) {
        g = g0[tri(i, c)];
        if (c == i) g = fma(og, A.se_full ? A.se[(size_t)i * m + i] : A.se[i], g);
        else if (A.se_full) g = fma(og, A.se[(size_t)i * m + c], g);
      }
      G[tri(i, c)] = g;
    }
  __syncthreads();
  if (!cholesky_packed(G, m, tid)) {
    for (int k = tid; k < n; k += THREADS) xnew[k] = quiet_nan();
    if (tid == 0) {
      A.status[prof] = 2;
      if (A.chi2) A.chi2[prof] = quiet_nan();
      if (A.nobs) A.nobs[prof] = m_used;
    }
    return;
  }

  // ---- 5: the two triangular solves, in wave 0's registers ----
  if (wave == 0) {
    double v0 = lane < m ? dvec[lane] : 0.0;
    double v1 = lane + 64 < m ? dvec[lane + 64] : 0.0;
    double v2 = lane + 128 < m ? dvec[lane + 128] : 0.0;
    solve_lower(G, m, lane, v0, v1, v2);
    const double chi2 = wave_sum(fma(v0, v0, fma(v1, v1, v2 * v2)));
    if (lane == 0 && A.chi2) A.chi2[prof] = chi2;
    solve_upper(G, m, lane, v0, v1, v2);
    if (lane < m) uvec[lane] = v0;
    if (lane + 64 < m) uvec[lane + 64] = v1;
    if (lane + 128 < m) uvec[lane + 128] = v2;
  }
  __syncthreads();

  // ---- 6: v = K^T u, x+ = xa + gamma / (1 + gamma) (x - xa) + Sa v ----
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
    xnew[j] = xap[j] + fma(wdx, xp[j] - xap[j], acc);
  }
  if (tid == 0) {
    A.status[prof] = 1;
    if (A.nobs) A.nobs[prof] = m_used;
  }
}

// ---- the cost at a state, on the rows of a linearisation ----
__global__ void __launch_bounds__(THREADS)
k_lm_cost(const LmArgs L) {
  extern __shared__ double smem[];
  const OeArgs& A = L.o;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (L.active && L.active[prof] == 0) return;
  const int m = A.m, n = A.n;
  const CostPlan P = cost_plan(m, n, A.se_full);
  double* dx = smem + P.dx;
  double* rvec = smem + P.r;
  double* red = smem + P.red;
  int* keep = reinterpret_cast<int*>(smem + P.keep);
  double* S = smem + P.s;

  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  int bad = 0;
  for (int k = tid; k < n; k += THREADS) {
    const double xv = xp[k], xav = xap[k];
    bad |= !finite_f64(xv) || !finite_f64(xav);
    dx[k] = xv - xav;
  }
  for (int i = tid; i < m; i += THREADS) {
    const int kp = L.keep[(size_t)prof * m + i] != 0;
    const double yv = A.y[(size_t)prof * m + i], fv = A.fx[(size_t)prof * m + i];
    bad |= kp && (!finite_f64(yv) || !finite_f64(fv));
    keep[i] = kp;
    rvec[i] = kp ? yv - fv : 0.0;
  }
  if (__syncthreads_or(bad)) {             // a trial to reject, not an error
    if (tid == 0) {
      L.cost[prof] = plus_inf();
      if (L.cost_obs) L.cost_obs[prof] = plus_inf();
      if (L.cost_prior) L.cost_prior[prof] = plus_inf();
      if (A.status) A.status[prof] = 1;
    }
    return;
  }

  // the prior term: thread j owns (Sa^-1 dx)_j dx_j (Sa^-1 symmetric: column j read as row j, coalesced over j)
  double part = 0.0;
  for (int j = tid; j < n; j += THREADS) {
    const double* col = L.sa_inv + j;
    double acc = 0.0;
#pragma unroll 16
    for (int k = 0; k < n; ++k) acc = fma(col[(size_t)k * n], dx[k], acc);
    part = fma(acc, dx[j], part);
  }
  const double prior = block_sum(part, red, tid);

  // the observation term over the rows kept
  double obs;
  int notpd = 0;
  if (!A.se_full) {
    part = 0.0;
    for (int i = tid; i < m; i += THREADS) {
      if (!keep[i]) continue;
      const double s = A.se[i];
      if (!(s > 0.0)) notpd = 1;
      part += rvec[i] * rvec[i] / s;
    }
    notpd = __syncthreads_or(notpd);
    obs = block_sum(part, red, tid);
  } else {
    for (int i = tid >> 4; i < m; i += THREADS / 16)
      for (int c = tid & 15; c <= i; c += 16)
        S[tri(i, c)] = (keep[i] && keep[c]) ? A.se[(size_t)i * m + c] : (c == i ? 1.0 : 0.0);
    __syncthreads();
    notpd = !cholesky_packed(S, m, tid);
    if (!notpd && wave == 0) {
      double v0 = lane < m ? rvec[lane] : 0.0;
      double v1 = lane + 64 < m ? rvec[lane + 64] : 0.0;
      double v2 = lane + 128 < m ? rvec[lane + 128] : 0.0;
      solve_lower(S, m, lane, v0, v1, v2);
      const double zz = wave_sum(fma(v0, v0, fma(v1, v1, v2 * v2)));
      if (lane == 0) red[0] = zz;
    }
    __syncthreads();
    obs = red[0];
  }
  if (tid == 0) {
    const double nan = quiet_nan();
    L.cost[prof] = notpd ? nan : obs + prior;
    if (L.cost_obs) L.cost_obs[prof] = notpd ? nan : obs;
    if (L.cost_prior) L.cost_prior[prof] = notpd ? nan : prior;
    if (A.status) A.status[prof] = notpd ? 2 : 1;
  }
}

// The dynamic-LDS limit of a kernel is raised when a launch first needs more than it had on that device, so a repeat call
// of the same (or a smaller) size makes no attribute call -- nothing but the launch, which a capturing stream accepts.
template <typename Kernel>
hipError_t launch_raised(Kernel kernel, std::atomic<size_t>* raised, const LmArgs& a, int64_t nprof, size_t lds,
                         hipStream_t st) {
  if (lds > 64 * 1024) {
    constexpr int MAX_DEV = 64;
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

template <int MR>
hipError_t launch_prepare_mr(const LmArgs& a, int64_t nprof, size_t lds, hipStream_t st) {
  static std::atomic<size_t> raised[64];
  return launch_raised(k_lm_prepare<MR>, raised, a, nprof, lds, st);
}

}  // namespace

hipError_t launch_lm_prepare(const LmArgs& a, int64_t nprof, hipStream_t st) {
  const size_t lds = oe::lds_plan(a.o.m, a.o.n).total_bytes;
  switch ((a.o.m + oe::ROW_TILE - 1) / oe::ROW_TILE) {
    case 1: return launch_prepare_mr<1>(a, nprof, lds, st);
    case 2: return launch_prepare_mr<2>(a, nprof, lds, st);
    case 3: return launch_prepare_mr<3>(a, nprof, lds, st);
    case 4: return launch_prepare_mr<4>(a, nprof, lds, st);
    case 5: return launch_prepare_mr<5>(a, nprof, lds, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_lm_solve(const LmArgs& a, int64_t nprof, hipStream_t st) {
  static std::atomic<size_t> raised[64];
  if (a.o.m > MWRT_OE_MAX_M) return hipErrorInvalidValue;
  return launch_raised(k_lm_solve, raised, a, nprof, solve_plan(a.o.m, a.o.n).total_bytes, st);
}

hipError_t launch_lm_cost(const LmArgs& a, int64_t nprof, hipStream_t st) {
  static std::atomic<size_t> raised[64];
  if (a.o.m > MWRT_OE_MAX_M) return hipErrorInvalidValue;
  return launch_raised(k_lm_cost, raised, a, nprof, cost_plan(a.o.m, a.o.n, a.o.se_full).total_bytes, st);
}

}  // namespace lm
}  // namespace mwrt
