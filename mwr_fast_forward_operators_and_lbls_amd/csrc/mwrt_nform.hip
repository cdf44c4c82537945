// mwrt_nform.hip -- the optimal-estimation step in the n-form (include/mwrt.h mwrt_oe_nform_*_device).  With
// r = y - F(x), W = diag(1 / se_i) over the rows kept and a damping factor gamma >= 0 per profile,
//     H = K^T W K,  g = K^T W r,     C = H + (1 + gamma) Sa^-1 = L L^T,     x+ = x + C^-1 [ g - Sa^-1 (x - xa) ]
// is Rodgers 2000, eq. 5.36 as printed; gamma = 0 is the step of csrc/mwrt_oe.hip and C^-1 its posterior covariance.  The
// system is n x n (n <= 128), so m is not bounded: nothing of size m x m exists.
//   k_nf_normal<TT>  the row rule, H, g and r^T W r in ONE pass over K -> caller-owned HBM; a thread owns TT 4 x 4 tiles of H
//   k_nf_solve       C in LDS, Cholesky, the two triangular solves, x+; at gamma = 0 chi2, dfs, diag C^-1 and C^-1
//   k_nf_cost        J = sum_kept (y - F)^2 / se + dx^T Sa^-1 dx at a state
// One workgroup of 256 threads per profile in all three; every sum has a fixed order and nothing is shared between
// workgroups, so a profile's outputs depend on neither its batch-mates nor nprof.  The factorisation, the solves, the
// inverse of the factor and the sums are the blocks of mwrt_oe_blocks.hip.h, unchanged.
#include "mwrt_nform.hip.h"
#include "mwrt_oe_blocks.hip.h"

#include <math.h>

namespace mwrt {
namespace nf {

namespace {

using namespace oe;                        // the blocks; THREADS is the same constant in both namespaces

constexpr int ROWS_PER_WAVE = ROW_CHUNK / (THREADS / 64);

// the row of packed entry e: e = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ int tri_row(int e) {
  int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > e) --i;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  return i;
}

// One chunk of ROW_CHUNK rows in registers, a wave per row (rows wave * 4 .. wave * 4 + 3 of the chunk) and lane l on the
// columns l and l + 64 of [K_0 | K_1 | ...], with the row's y, F and variance in every lane.
struct Stage {
  double k[ROWS_PER_WAVE][2];
  double y[ROWS_PER_WAVE], f[ROWS_PER_WAVE], s[ROWS_PER_WAVE];

  __device__ __forceinline__ void fetch(const double* const (&col)[2], const bool (&cin)[2], const double* yp, const double* fp,
                                        const double* sep, int64_t r0, int m, int nlev, int wave) {
#pragma unroll
    for (int q = 0; q < ROWS_PER_WAVE; ++q) {
      const int64_t row = r0 + wave * ROWS_PER_WAVE + q;
      const bool in = row < m;
#pragma unroll
      for (int h = 0; h < 2; ++h) k[q][h] = (in && cin[h]) ? col[h][(size_t)row * nlev] : 0.0;
      y[q] = in ? yp[row] : 0.0;
      f[q] = in ? fp[row] : 0.0;
      s[q] = in ? sep[row] : 1.0;
    }
  }

  // The row rule on what was fetched (the select after the load: a dropped row may hold NaN), then the rows to LDS: Ks the
  // row, Kw the row times 1 / se_i, both 0 for a dropped row and in the columns n .. pitch - 1.  `kept` and `bad` count the
  // wave's rows kept and those among them whose variance is not > 0.
  __device__ __forceinline__ void store(double* Ks, double* Kw, double* res, double* wres, uint8_t* keepout, int64_t r0, int m,
                                        int pitch, int wave, int lane, int& kept, int& bad) const {
#pragma unroll
    for (int q = 0; q < ROWS_PER_WAVE; ++q) {
      const int lr = wave * ROWS_PER_WAVE + q;
      const int64_t row = r0 + lr;
      const bool in = row < m;
      const bool ok = finite_f64(k[q][0]) && finite_f64(k[q][1]) && finite_f64(y[q]) && finite_f64(f[q]) && finite_f64(s[q]);
      const bool keep = __all(ok) && in;
      const double w = 1.0 / s[q];
      const double dy = y[q] - f[q];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        if (c < pitch) {
          Ks[lr * pitch + c] = keep ? k[q][h] : 0.0;
          Kw[lr * pitch + c] = keep ? k[q][h] * w : 0.0;
        }
      }
      if (lane == 0) {
        res[lr] = keep ? dy : 0.0;
        wres[lr] = keep ? dy * w : 0.0;
        if (in) keepout[row] = keep ? 1 : 0;
      }
      kept += keep ? 1 : 0;
      bad += (keep && !(s[q] > 0.0)) ? 1 : 0;
    }
  }
};

// ---- the linearisation: H = K^T W K, g = K^T W r, r^T W r, the rows kept ----
template <int TT>
__global__ void __launch_bounds__(THREADS)
k_nf_normal(const NfArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (A.active && A.active[prof] == 0) return;
  const int m = A.m, n = A.n, nlev = A.nlev;
  const NormalPlan P = normal_plan(n);
  const int pitch = P.pitch;
  double* Ks = smem + P.ks;
  double* Kw = smem + P.kw;
  double* res = smem + P.res;
  double* wres = smem + P.wres;
  int* counts = reinterpret_cast<int*>(smem + P.counts);

  const int nt = n * (n + 1) / 2;
  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  double* hout = A.h + (size_t)prof * nt;
  double* gout = A.g + (size_t)prof * n;
  uint8_t* keepout = A.keep + (size_t)prof * m;

  // ---- 1: the state ----
  if (state_bad<false>(xp, xap, n, nullptr, tid)) {
    for (int e = tid; e < nt; e += THREADS) hout[e] = quiet_nan();
    for (int j = tid; j < n; j += THREADS) gout[j] = quiet_nan();
    for (int64_t i = tid; i < m; i += THREADS) keepout[i] = 0;
    if (tid == 0) {
      A.rwr[prof] = quiet_nan();
      A.nobs[prof] = 0;
      A.lin_status[prof] = 0;
    }
    return;
  }

  // the lane's two columns of [K_0 | K_1 | ...]
  const double* col[2];
  bool cin[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    cin[h] = c < n;
    const int b = cin[h] ? c / nlev : 0;
    const double* base = b == 0 ? A.k0 : b == 1 ? A.k1 : b == 2 ? A.k2 : A.k3;
    col[h] = base + (size_t)prof * m * nlev + (cin[h] ? c - b * nlev : 0);
  }
  const double* yp = A.y + (size_t)prof * m;
  const double* fp = A.fx + (size_t)prof * m;
  const double* sep = A.se + (A.se_per_profile ? (size_t)prof * m : 0);

  // the thread's tiles (bi < 0: none), the column of g it sums (THREADS - 1 - tid: the threads with the fewest tiles)
  const int ntiles = tile_count(n);
  int bi[TT], bj[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const int tile = tid + THREADS * t;
    bi[t] = tile < ntiles ? tri_row(tile) : -1;
    bj[t] = tile < ntiles ? tile - bi[t] * (bi[t] + 1) / 2 : 0;
  }
  const int gj = THREADS - 1 - tid;
  double acc[TT][TILE][TILE];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
      for (int c = 0; c < TILE; ++c) acc[t][a][c] = 0.0;
  double gacc = 0.0, racc = 0.0;
  int kept = 0, bad = 0;

  // ---- 2 and 3: the row rule as the rows are staged, the sums over the rows in ascending order ----
  Stage st;
  st.fetch(col, cin, yp, fp, sep, 0, m, nlev, wave);
  for (int64_t r0 = 0; r0 < m; r0 += ROW_CHUNK) {
    st.store(Ks, Kw, res, wres, keepout, r0, m, pitch, wave, lane, kept, bad);
    __syncthreads();
    if (r0 + ROW_CHUNK < m) st.fetch(col, cin, yp, fp, sep, r0 + ROW_CHUNK, m, nlev, wave);   // in flight during the sums
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (bi[t] < 0) continue;
      const double* wrow = Kw + TILE * bi[t];
      const double* krow = Ks + TILE * bj[t];
#pragma unroll 4
      for (int r = 0; r < ROW_CHUNK; ++r) {
        double a[TILE], q[TILE];
#pragma unroll
        for (int u = 0; u < TILE; ++u) a[u] = wrow[r * pitch + u];
#pragma unroll
        for (int u = 0; u < TILE; ++u) q[u] = krow[r * pitch + u];
#pragma unroll
        for (int u = 0; u < TILE; ++u)
#pragma unroll
          for (int c = 0; c < TILE; ++c) acc[t][u][c] = fma(a[u], q[c], acc[t][u][c]);
      }
    }
    if (gj < n) {
#pragma unroll 4
      for (int r = 0; r < ROW_CHUNK; ++r) gacc = fma(Kw[r * pitch + gj], res[r], gacc);
    } else if (gj == n) {
#pragma unroll 4
      for (int r = 0; r < ROW_CHUNK; ++r) racc = fma(res[r], wres[r], racc);
    }
    __syncthreads();
  }

  if (lane == 0) {
    counts[wave] = kept;
    counts[THREADS / 64 + wave] = bad;
  }
  __syncthreads();
  int m_used = 0, nbad = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    m_used += counts[w];
    nbad += counts[THREADS / 64 + w];
  }
  const int status = m_used == 0 ? 3 : nbad != 0 ? 2 : 1;      // nothing kept: every sum is 0 as it stands
  const bool nan = status == 2;
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    if (bi[t] < 0) continue;
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
      for (int c = 0; c < TILE; ++c) {
        const int i = TILE * bi[t] + a, j = TILE * bj[t] + c;
        if (i < n && j <= i) hout[tri(i, j)] = nan ? quiet_nan() : acc[t][a][c];
      }
  }
  if (gj < n) gout[gj] = nan ? quiet_nan() : gacc;
  else if (gj == n) A.rwr[prof] = nan ? quiet_nan() : racc;
  if (tid == 0) {
    A.nobs[prof] = m_used;
    A.lin_status[prof] = (uint8_t)status;
  }
}

// every output of a solve that failed: NaN
__device__ __forceinline__ void solve_failed(const NfArgs& A, int64_t prof, int status, int tid) {
  const int n = A.n;
  for (int k = tid; k < n; k += THREADS) {
    A.x_new[(size_t)prof * n + k] = quiet_nan();
    if (A.post_var) A.post_var[(size_t)prof * n + k] = quiet_nan();
  }
  if (A.post_cov)
    for (int e = tid; e < n * n; e += THREADS) A.post_cov[(size_t)prof * n * n + e] = quiet_nan();
  if (tid == 0) {
    A.status[prof] = (uint8_t)status;
    if (A.chi2) A.chi2[prof] = quiet_nan();
    if (A.dfs) A.dfs[prof] = quiet_nan();
  }
}

// ---- one (optionally damped) step on a linearisation ----
__global__ void __launch_bounds__(THREADS)
k_nf_solve(const NfArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (A.active && A.active[prof] == 0) return;
  const int n = A.n;
  const SolvePlan P = solve_plan(n);
  double* C = smem + P.c;
  double* rhs = smem + P.rhs;
  double* sv = smem + P.s;
  double* dx = smem + P.dx;
  double* de = smem + P.de;
  double* red = smem + P.red;

  const int nt = n * (n + 1) / 2;
  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  const double* hin = A.h + (size_t)prof * nt;
  const double* gin = A.g + (size_t)prof * n;
  double* xnew = A.x_new + (size_t)prof * n;
  const double gamma = A.gamma ? A.gamma[prof] : 0.0;
  const int lin = A.lin_status[prof];
  const bool gamma_ok = finite_f64(gamma) && gamma >= 0.0;
  const double og = 1.0 + gamma;           // >= 1 when gamma_ok
  const bool want_inverse = A.dfs || A.post_var || A.post_cov;

  const bool state = state_bad<true>(xp, xap, n, dx, tid);
  if (state || lin == 0) { solve_failed(A, prof, 0, tid); return; }
  if (!gamma_ok || (lin != 1 && lin != 3)) { solve_failed(A, prof, 2, tid); return; }
  const bool nothing = lin == 3;           // no usable row: H = 0 and g = 0, whatever the buffers hold
  if (nothing) {                           // the damped pull towards the prior alone, xa exactly at gamma = 0
    const double wdx = gamma / og;
    for (int k = tid; k < n; k += THREADS) xnew[k] = gamma == 0.0 ? xap[k] : xap[k] + wdx * dx[k];
    if (tid == 0) {
      A.status[prof] = 3;
      if (A.chi2) A.chi2[prof] = 0.0;
      if (A.dfs) A.dfs[prof] = 0.0;
    }
    if (!A.post_var && !A.post_cov) return;
  }

  // ---- C = H + (1 + gamma) Sa^-1, the right-hand side g - Sa^-1 (x - xa); Cholesky ----
  for (int i = tid >> 4; i < n; i += THREADS / 16)
    for (int c = tid & 15; c <= i; c += 16)
      C[tri(i, c)] = fma(og, A.sa_inv[(size_t)i * n + c], nothing ? 0.0 : hin[tri(i, c)]);
  if (!nothing)
    for (int i = tid; i < n; i += THREADS) rhs[i] = gin[i] - sa_times(A.sa_inv, n, i, dx);
  __syncthreads();
  if (!cholesky_packed(C, n, tid)) {
    if (!nothing) { solve_failed(A, prof, 2, tid); return; }
    for (int k = tid; k < n; k += THREADS)
      if (A.post_var) A.post_var[(size_t)prof * n + k] = quiet_nan();
    if (A.post_cov)
      for (int e = tid; e < n * n; e += THREADS) A.post_cov[(size_t)prof * n * n + e] = quiet_nan();
    return;
  }

  if (!nothing) {
    // ---- the two triangular solves, in wave 0's registers; x+ = x + s ----
    if (wave == 0) (void)solve_llt(C, rhs, sv, n, lane);
    __syncthreads();
    for (int k = tid; k < n; k += THREADS) {
      const double xn = xp[k] + sv[k];
      xnew[k] = xn;
      de[k] = xn - xap[k];
    }
    if (tid == 0) A.status[prof] = 1;
    __syncthreads();

    // ---- chi2 as the cost at the linear solution: (r^T W r - 2 s^T g + s^T H s) + e^T Sa^-1 e ----
    if (A.chi2) {
      double sg = 0.0, shs = 0.0, prior = 0.0;
      for (int i = tid; i < n; i += THREADS) {
        double hs = 0.0;
        for (int j = 0; j < n; ++j) hs = fma(hin[j <= i ? tri(i, j) : tri(j, i)], sv[j], hs);
        sg = fma(sv[i], gin[i], sg);
        shs = fma(sv[i], hs, shs);
        prior = fma(sa_times(A.sa_inv, n, i, de), de[i], prior);
      }
      sg = block_sum(sg, red, tid);
      shs = block_sum(shs, red, tid);
      prior = block_sum(prior, red, tid);
      if (tid == 0) A.chi2[prof] = (A.rwr[prof] - 2.0 * sg + shs) + prior;
    }
  }

  // ---- C^-1 = L^-T L^-1 from the inverted factor: its diagonal, all of it, and tr(C^-1 H) ----
  if (want_inverse) {
    invert_lower(C, n, tid);
    double part = 0.0;
    for (int e = tid; e < nt; e += THREADS) {
      const int i = tri_row(e), j = e - i * (i + 1) / 2;
      double cinv = 0.0;
      for (int k = i; k < n; ++k) cinv = fma(C[tri(k, i)], C[tri(k, j)], cinv);
      if (A.post_cov) {
        A.post_cov[(size_t)prof * n * n + (size_t)i * n + j] = cinv;
        A.post_cov[(size_t)prof * n * n + (size_t)j * n + i] = cinv;
      }
      if (A.post_var && i == j) A.post_var[(size_t)prof * n + i] = cinv;
      if (A.dfs && !nothing) part = fma(i == j ? cinv : 2.0 * cinv, hin[e], part);
    }
    if (A.dfs && !nothing) {
      const double dfs = block_sum(part, red, tid);
      if (tid == 0) A.dfs[prof] = dfs;
    }
  }
}

// ---- the cost at a state, on the rows of a linearisation ----
__global__ void __launch_bounds__(THREADS)
k_nf_cost(const NfArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x;
  const int64_t prof = blockIdx.x;
  if (A.active && A.active[prof] == 0) return;
  const int m = A.m, n = A.n;
  const CostPlan P = cost_plan(n);
  double* dx = smem + P.dx;
  double* red = smem + P.red;

  const double* xp = A.x + (size_t)prof * n;
  const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
  const double* yp = A.y + (size_t)prof * m;
  const double* fp = A.fx + (size_t)prof * m;
  const double* sep = A.se + (A.se_per_profile ? (size_t)prof * m : 0);
  const uint8_t* keep = A.keep + (size_t)prof * m;

  // the observation term: thread t sums its rows t, t + 256, ... in ascending order, then the fixed tree
  int bad = state_scan<true>(xp, xap, n, dx, tid);
  int notpd = 0;
  double part = 0.0;
  for (int64_t i = tid; i < m; i += THREADS) {
    if (keep[i] == 0) continue;
    const double yv = yp[i], fv = fp[i], s = sep[i];
    bad |= !finite_f64(yv) || !finite_f64(fv);
    if (!(s > 0.0)) notpd = 1;
    const double d = yv - fv;
    part += d * d / s;
  }
  if (__syncthreads_or(bad)) {             // a trial to reject, not an error
    if (tid == 0) {
      A.cost[prof] = plus_inf();
      if (A.cost_obs) A.cost_obs[prof] = plus_inf();
      if (A.cost_prior) A.cost_prior[prof] = plus_inf();
      if (A.status) A.status[prof] = 1;
    }
    return;
  }
  notpd = __syncthreads_or(notpd);
  const double obs = block_sum(part, red, tid);

  // the prior term: thread j owns (Sa^-1 dx)_j dx_j
  part = 0.0;
  for (int j = tid; j < n; j += THREADS) part = fma(sa_times(A.sa_inv, n, j, dx), dx[j], part);
  const double prior = block_sum(part, red, tid);
  if (tid == 0) {
    const double nan = quiet_nan();
    A.cost[prof] = notpd ? nan : obs + prior;
    if (A.cost_obs) A.cost_obs[prof] = notpd ? nan : obs;
    if (A.cost_prior) A.cost_prior[prof] = notpd ? nan : prior;
    if (A.status) A.status[prof] = notpd ? 2 : 1;
  }
}

}  // namespace

hipError_t launch_nf_normal(const NfArgs& a, int64_t nprof, hipStream_t st) {
  if (a.n > MWRT_OE_NFORM_MAX_N) return hipErrorInvalidValue;
  const size_t lds = normal_plan(a.n).total_bytes;
  switch (tiles_per_thread(a.n)) {
    case 1: return launch_raised<k_nf_normal<1>>(a, nprof, lds, st);
    case 2: return launch_raised<k_nf_normal<2>>(a, nprof, lds, st);
    case 3: return launch_raised<k_nf_normal<3>>(a, nprof, lds, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_nf_solve(const NfArgs& a, int64_t nprof, hipStream_t st) {
  if (a.n > MWRT_OE_NFORM_MAX_N) return hipErrorInvalidValue;
  return launch_raised<k_nf_solve>(a, nprof, solve_plan(a.n).total_bytes, st);
}

hipError_t launch_nf_cost(const NfArgs& a, int64_t nprof, hipStream_t st) {
  if (a.n > MWRT_OE_NFORM_MAX_N) return hipErrorInvalidValue;
  return launch_raised<k_nf_cost>(a, nprof, cost_plan(a.n).total_bytes, st);
}

}  // namespace nf
}  // namespace mwrt
