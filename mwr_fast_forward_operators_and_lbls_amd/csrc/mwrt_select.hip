// mwrt_select.hip -- observation selection by information content (include/mwrt.h mwrt_oe_select_device, DESIGN 4.12;
// Rodgers 2000, section 2.5; Rabier et al. 2002).  Per profile, with rows k_i of [K0 | K1 | ...], variances se_i and a
// start covariance S0, the greedy sequence that takes in every round the unchosen candidate of the largest
//     q_i = k_i^T S k_i / se_i            (entropy reduction log2(1 + q_i) / 2)
// and then assimilates it: v = S k_j, d = se_j + k_j^T v, S <- S - v v^T / d, q_i <- max(0, q_i - (k_i^T v)^2 / (d se_i)).
//   k_sel_select   one workgroup per profile.  S stays in LDS as a packed lower triangle for the whole selection; q and
//                  rank live in global memory (m is not bounded).  A pass over K is a wave per row, a lane per state
//                  element (and element + 64): the initial pass forms k_i^T S0 k_i against S in LDS, the pass of a round
//                  k_i^T v, and either keeps the wave's best row on the way, so the argmax costs no pass of its own.  A
//                  wave issues the loads of ROWS_IN_FLIGHT rows (K, q, rank, se) before it works on the first: a row's
//                  work is a short dependent chain behind its loads, and with one row at a time the pass waits for
//                  memory once per row.  K is read nsel + 1 times, every row every time (the select comes after the
//                  load); the last pass leaves in q what every unchosen candidate would still add.
// No atomics, no MFMA, no workspace, no scratch.  Every sum has the fixed order mwrt_select.hip.h states: a row's q depends
// on its values alone, never on its index, so two identical rows tie exactly and the lower index wins.  The blocks of
// mwrt_oe_blocks.hip.h are used unchanged.  Every global index is 64-bit.
#include "mwrt_select.hip.h"
#include "mwrt_oe_blocks.hip.h"

#include <math.h>

namespace mwrt {
namespace sel {

namespace {

using namespace oe;                        // the blocks; THREADS is the same constant in both namespaces

// A lane's two elements of a row of [K0 | K1 | ...]: where they start in the profile's blocks, and whether they exist.
struct Cols {
  const double* p0; const double* p1;      // element lane (lane + 64) of row 0 of this profile
  bool in0, in1;
};
__device__ __forceinline__ Cols lane_cols(const SelArgs& A, int64_t prof, int lane) {
  Cols c;
  c.in0 = lane < A.n;
  c.in1 = lane + 64 < A.n;
  const int e0 = c.in0 ? lane : 0, e1 = c.in1 ? lane + 64 : 0;
  const int b0 = e0 / A.nlev, b1 = e1 / A.nlev;
  const size_t base = (size_t)prof * A.m * A.nlev;
  c.p0 = (b0 == 0 ? A.k0 : b0 == 1 ? A.k1 : b0 == 2 ? A.k2 : A.k3) + base + (e0 - b0 * A.nlev);
  c.p1 = (b1 == 0 ? A.k0 : b1 == 1 ? A.k1 : b1 == 2 ? A.k2 : A.k3) + base + (e1 - b1 * A.nlev);
  return c;
}
__device__ __forceinline__ void load_row(const SelArgs& A, const Cols& c, int i, bool two, double& a0, double& a1) {
  const size_t off = (size_t)i * A.nlev;
  a0 = c.in0 ? c.p0[off] : 0.0;
  a1 = (two && c.in1) ? c.p1[off] : 0.0;
}

// the wave's best row so far (lane-uniform): a strict maximum in ascending row order keeps the lowest index
struct Best {
  double q; int i;
  __device__ __forceinline__ void see(double qi, int row) { if (qi > q) { q = qi; i = row; } }
};

// `v` into every floating-point output of the profile, -1 into order and rank, 0 into count.  The caller stands behind a
// barrier that no write of the selection can pass.
__device__ __forceinline__ void fail_outputs(const SelArgs& A, int64_t prof, double v, int tid) {
  const int n = A.n;
  for (int t = tid; t < A.nsel; t += THREADS) {
    A.order[(size_t)prof * A.nsel + t] = -1;
    A.q_pick[(size_t)prof * A.nsel + t] = v;
    if (A.dfs_gain) A.dfs_gain[(size_t)prof * A.nsel + t] = v;
  }
  for (int i = tid; i < A.m; i += THREADS) {
    A.rank[(size_t)prof * A.m + i] = -1;
    A.q[(size_t)prof * A.m + i] = v;
  }
  if (A.post_cov)
    for (int e = tid; e < n * n; e += THREADS) A.post_cov[(size_t)prof * n * n + e] = v;
  if (A.post_var)
    for (int k = tid; k < n; k += THREADS) A.post_var[(size_t)prof * n + k] = v;
  if (tid == 0) A.count[prof] = 0;
}

// the four waves' bests compared in wave order; every thread gets the same answer.  Ends behind a barrier.
__device__ __forceinline__ Best block_best(const Best& mine, double* bq, int* bi, int lane, int wave) {
  if (lane == 0) { bq[wave] = mine.q; bi[wave] = mine.i; }
  __syncthreads();
  Best b{bq[0], bi[0]};
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    const double qw = bq[w];
    const int iw = bi[w];
    if (qw > b.q || (qw == b.q && iw >= 0 && (b.i < 0 || iw < b.i))) { b.q = qw; b.i = iw; }
  }
  __syncthreads();
  return b;
}

__global__ void __launch_bounds__(THREADS)
k_sel_select(const SelArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform, and known to be: row indices stay scalar
  const int64_t prof = blockIdx.x;
  if (A.active && A.active[prof] == 0) return;
  const int n = A.n, m = A.m, nsel = A.nsel;
  const SelPlan P = sel_plan(n);
  double* S = smem + P.s;
  double* vv = smem + P.v;
  double* uu = smem + P.u;
  double* kj = smem + P.kj;                // k_j; once d is known, w = Sa^-1 v
  double* bq = smem + P.best;
  int* bi = reinterpret_cast<int*>(smem + P.ints);
  int* nc = bi + WAVES;

  const double* s0 = A.s0 + (A.s0_per_profile ? (size_t)prof * n * n : 0);
  const double* sep = A.se + (A.se_per_profile ? (size_t)prof * m : 0);
  const uint8_t* keep = A.keep ? A.keep + (size_t)prof * m : nullptr;
  double* q = A.q + (size_t)prof * m;
  int32_t* rank = A.rank + (size_t)prof * m;
  int32_t* order = A.order + (size_t)prof * nsel;
  double* q_pick = A.q_pick + (size_t)prof * nsel;
  double* dfs_gain = A.dfs_gain ? A.dfs_gain + (size_t)prof * nsel : nullptr;

  // ---- S0 into LDS (its lower triangle), finiteness of all of it and of Sa^-1 when that is read ----
  int bad = 0;
  for (int e = tid; e < n * n; e += THREADS) {
    const double s = s0[e];
    bad |= !finite_f64(s);
    if (dfs_gain) bad |= !finite_f64(A.sa_inv[e]);
    const int i = e / n, c = e - i * n;
    if (c <= i) S[tri(i, c)] = s;
  }
  if (__syncthreads_or(bad)) {
    fail_outputs(A, prof, quiet_nan(), tid);
    if (tid == 0) A.status[prof] = 0;
    return;
  }

  const bool two = n > 64;                                     // uniform: the second element of a lane exists
  const Cols C = lane_cols(A, prof, lane);
  const int c0 = C.in0 ? lane : 0, c1 = C.in1 ? lane + 64 : 0;   // a lane beyond n reads column 0 and adds nothing
  const int t0 = c0 * (c0 + 1) / 2, t1 = c1 * (c1 + 1) / 2;

  // ---- the candidates and q_i = k_i^T S0 k_i / se_i ----
  Best mine{0.0, -1};
  int ncand = 0, badvar = 0;
  for (int64_t i64 = wave; i64 < m; i64 += WAVES) {          // one row at a time: the n fused multiply-adds behind the
    const int i = (int)i64;                                    // loads outweigh the wait for them
    double a0, a1;
    load_row(A, C, i, two, a0, a1);
    const double sei = sep[i];
    bool ok = finite_f64(a0) && finite_f64(a1) && finite_f64(sei);
    ok = __all(ok) && (!keep || keep[i] != 0) && (!A.candidate || A.candidate[i] != 0);   // the select after the load
    double qi = 0.0;
    if (ok) {
      ++ncand;
      if (!(sei > 0.0)) {
        badvar = 1;
      } else {
        double y0 = 0.0, y1 = 0.0;
        for (int l = 0; l < n; ++l) {
          const double kl = __shfl(l < 64 ? a0 : a1, l & 63);
          const int tl = l * (l + 1) / 2;
          y0 = fma(S[c0 >= l ? t0 + l : tl + c0], kl, y0);
          if (two) y1 = fma(S[c1 >= l ? t1 + l : tl + c1], kl, y1);
        }
        double part = a0 * y0;
        if (two) part = fma(a1, y1, part);
        qi = wave_sum(part) / sei;
        mine.see(qi, i);
      }
    }
    if (lane == 0) { q[i] = qi; rank[i] = -1; }
  }
  if (lane == 0) nc[wave] = ncand;
  if (__syncthreads_or(badvar)) {                              // a candidate's variance is <= 0
    fail_outputs(A, prof, quiet_nan(), tid);
    if (tid == 0) A.status[prof] = 2;
    return;
  }
  int candidates = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) candidates += nc[w];

  // ---- the rounds ----
  int t = 0;
  for (; t < nsel; ++t) {
    const Best b = block_best(mine, bq, bi, lane, wave);
    if (!(b.q > 0.0)) break;                                   // uniform: nothing left that adds information
    const int j = b.i;
    const double sej = sep[j];
    for (int k = tid; k < n; k += THREADS) {
      const int blk = k / A.nlev;
      const double* kb = blk == 0 ? A.k0 : blk == 1 ? A.k1 : blk == 2 ? A.k2 : A.k3;
      kj[k] = kb[((size_t)prof * m + j) * A.nlev + (k - blk * A.nlev)];
    }
    __syncthreads();
    for (int c = tid; c < n; c += THREADS) {                   // v = S k_j
      const int tc = c * (c + 1) / 2;
      double acc = 0.0;
      for (int l = 0; l < n; ++l) acc = fma(S[c >= l ? tc + l : l * (l + 1) / 2 + c], kj[l], acc);
      vv[c] = acc;
    }
    __syncthreads();
    const double v0 = C.in0 ? vv[c0] : 0.0, v1 = C.in1 ? vv[c1] : 0.0;
    double part = (C.in0 ? kj[c0] : 0.0) * v0;
    if (two) part = fma(C.in1 ? kj[c1] : 0.0, v1, part);
    const double d = sej + wave_sum(part);                     // every wave forms the same d
    if (!(d > 0.0) || !finite_f64(d)) {
      __syncthreads();
      fail_outputs(A, prof, quiet_nan(), tid);
      if (tid == 0) A.status[prof] = 2;
      return;
    }
    __syncthreads();                                           // k_j is read; its place takes w
    if (dfs_gain) {
      for (int c = tid; c < n; c += THREADS) kj[c] = sa_times(A.sa_inv, n, c, vv);
      __syncthreads();
      double g = v0 * (C.in0 ? kj[c0] : 0.0);
      if (two) g = fma(v1, C.in1 ? kj[c1] : 0.0, g);
      g = wave_sum(g) / d;
      if (tid == 0) dfs_gain[t] = g;
    }
    if (tid == 0) { order[t] = j; q_pick[t] = b.q; rank[j] = t; }
    for (int c = tid; c < n; c += THREADS) uu[c] = vv[c] / d;
    __syncthreads();                                           // u, and rank[j] for the wave that owns row j
    for (int i = tid >> 4; i < n; i += THREADS / 16) {         // S <- S - v v^T / d
      const double ui = -uu[i];
      for (int c = tid & 15; c <= i; c += 16) S[tri(i, c)] = fma(ui, vv[c], S[tri(i, c)]);
    }
    // q_i of the rows still in play, and the wave's best of them
    mine = Best{0.0, -1};
    for (int64_t i0 = wave; i0 < m; i0 += WAVES * ROWS_IN_FLIGHT) {
      double a0[ROWS_IN_FLIGHT], a1[ROWS_IN_FLIGHT], sev[ROWS_IN_FLIGHT], qv[ROWS_IN_FLIGHT];
      int rk[ROWS_IN_FLIGHT];
#pragma unroll
      for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {               // the loads of the group first, whatever q and rank will say
        const int i = (int)(i0 + u * WAVES < m ? i0 + u * WAVES : m - 1);
        qv[u] = q[i];
        rk[u] = rank[i];
        sev[u] = sep[i];
        load_row(A, C, i, two, a0[u], a1[u]);
      }
#pragma unroll
      for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
        if (i0 + u * WAVES >= m) break;                        // uniform
        const int i = (int)(i0 + u * WAVES);
        const double qi = qv[u];
        if (rk[u] >= 0 || qi == 0.0) continue;                 // uniform; a row that is no candidate holds exact 0.0: its
        double dot = a0[u] * v0;                               // values were loaded and are never used
        if (two) dot = fma(a1[u], v1, dot);
        dot = wave_sum(dot);
        const double qn = fmax(0.0, qi - dot * dot / (d * sev[u]));
        if (lane == 0) q[i] = qn;
        mine.see(qn, i);
      }
    }
    __syncthreads();                                           // S is updated, v and u are free
  }
  for (int r = t + tid; r < nsel; r += THREADS) {
    order[r] = -1;
    q_pick[r] = 0.0;
    if (dfs_gain) dfs_gain[r] = 0.0;
  }
  if (A.post_cov)
    for (int e = tid; e < n * n; e += THREADS) {
      const int i = e / n, c = e - i * n;
      A.post_cov[(size_t)prof * n * n + e] = S[c <= i ? tri(i, c) : tri(c, i)];
    }
  if (A.post_var)
    for (int k = tid; k < n; k += THREADS) A.post_var[(size_t)prof * n + k] = S[tri(k, k)];
  if (tid == 0) {
    A.count[prof] = t;
    A.status[prof] = candidates == 0 ? 3 : 1;
  }
}

}  // namespace

hipError_t launch_select(const SelArgs& a, int64_t nprof, hipStream_t st) {
  if (a.n > MWRT_OE_NFORM_MAX_N) return hipErrorInvalidValue;
  return launch_raised<k_sel_select>(a, nprof, sel_plan(a.n).total_bytes, st);
}

}  // namespace sel
}  // namespace mwrt
