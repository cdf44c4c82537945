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
// workgroups, so a profile's outputs depend on neither its batch-mates nor nprof.  Every step the three have in common with
// k_oe_step is that kernel's block (mwrt_oe_blocks.hip.h; DESIGN 4.6 lists them).
#include "mwrt_oe_lm.hip.h"
#include "mwrt_oe_blocks.hip.h"

#include <math.h>

namespace mwrt {
namespace lm {

namespace {

using namespace oe;                        // the blocks; THREADS is the same constant in both namespaces

// ---- the linearisation: G0 = K Sa K^T, r = y - F(x), K (x - xa), the rows kept ----
template <int MR>
__global__ void __launch_bounds__(THREADS)
k_lm_prepare(const LmArgs L) {
  extern __shared__ double smem[];
  const OeArgs& A = L.o;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (L.active && L.active[prof] == 0) return;
  const int m = A.m, n = A.n;
  const LdsPlan P = lds_plan(m, n);
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
  if (state_bad<true>(xp, xap, n, vbuf, tid)) {
    for (int i = tid; i < m; i += THREADS) { rout[i] = quiet_nan(); kout[i] = quiet_nan(); keepout[i] = 0; }
    for (int e = tid; e < ng; e += THREADS) g0[e] = quiet_nan();
    if (tid == 0) L.lin_status[prof] = 0;
    return;
  }

  // ---- 2: rows ----
  for (int i = wave; i < mp; i += THREADS / 64) {
    const Row r = row_rule<true>(A, prof, i, vbuf, lane);
    if (lane == 0) {
      keep[i] = r.keep ? 1 : 0;
      if (i < m) {
        keepout[i] = r.keep ? 1 : 0;
        rout[i] = r.keep ? r.dy : 0.0;
        kout[i] = r.keep ? r.kdx : 0.0;
      }
    }
  }
  __syncthreads();
  if (rows_kept(keep, m) == 0) {           // nothing observed: G0 = 0
    for (int e = tid; e < ng; e += THREADS) g0[e] = 0.0;
    if (tid == 0) L.lin_status[prof] = 3;
    return;
  }

  // ---- 3: G0 = K Sa K^T ----
  form_G<MR>(A, prof, keep, G, Wt, Ks, Ss, kpitch);
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
  const int m = A.m, n = A.n;
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

  int bad = state_scan<false>(xp, xap, n, nullptr, tid);
  for (int i = tid; i < m; i += THREADS) {
    const int kp = L.keep[(size_t)prof * m + i] != 0;
    keep[i] = kp;
    dvec[i] = kp ? L.r[(size_t)prof * m + i] + L.kdx[(size_t)prof * m + i] / og : 0.0;
  }
  bad = __syncthreads_or(bad);
  const int m_used = rows_kept(keep, m);
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
  // Not add_se_and_identity_rows: G0 comes from HBM, Se_ii is read where it is used (no sed in this plan) and a dropped row
  // is written whole, whatever the caller's g0 holds there.
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
    const double chi2 = solve_llt(G, dvec, uvec, m, lane);
    if (lane == 0 && A.chi2) A.chi2[prof] = chi2;
  }
  __syncthreads();

  // ---- 6: v = K^T u, x+ = xa + gamma / (1 + gamma) (x - xa) + Sa v ----
  kt_u(A, prof, keep, uvec, vbuf, tid);
  for (int j = tid; j < n; j += THREADS) xnew[j] = xap[j] + fma(wdx, xp[j] - xap[j], sa_times(A.sa, n, j, vbuf));
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
  int bad = state_scan<true>(xp, xap, n, dx, tid);
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
  for (int j = tid; j < n; j += THREADS) part = fma(sa_times(L.sa_inv, n, j, dx), dx[j], part);
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

}  // namespace

hipError_t launch_lm_prepare(const LmArgs& a, int64_t nprof, hipStream_t st) {
  const size_t lds = lds_plan(a.o.m, a.o.n).total_bytes;
  switch ((a.o.m + ROW_TILE - 1) / ROW_TILE) {
    case 1: return launch_raised<k_lm_prepare<1>>(a, nprof, lds, st);
    case 2: return launch_raised<k_lm_prepare<2>>(a, nprof, lds, st);
    case 3: return launch_raised<k_lm_prepare<3>>(a, nprof, lds, st);
    case 4: return launch_raised<k_lm_prepare<4>>(a, nprof, lds, st);
    case 5: return launch_raised<k_lm_prepare<5>>(a, nprof, lds, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_lm_solve(const LmArgs& a, int64_t nprof, hipStream_t st) {
  if (a.o.m > MWRT_OE_MAX_M) return hipErrorInvalidValue;
  return launch_raised<k_lm_solve>(a, nprof, solve_plan(a.o.m, a.o.n).total_bytes, st);
}

hipError_t launch_lm_cost(const LmArgs& a, int64_t nprof, hipStream_t st) {
  if (a.o.m > MWRT_OE_MAX_M) return hipErrorInvalidValue;
  return launch_raised<k_lm_cost>(a, nprof, cost_plan(a.o.m, a.o.n, a.o.se_full).total_bytes, st);
}

}  // namespace lm
}  // namespace mwrt
