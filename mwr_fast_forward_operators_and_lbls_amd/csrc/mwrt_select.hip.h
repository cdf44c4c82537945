// mwrt_select.hip.h -- observation selection by information content (csrc/mwrt_select.hip): argument record,
// the LDS plan and the launcher only, as the host unit reads them.  No kernel lives here; the plan is host and device code
// so that launcher and kernel lay the block out by the same rule.
#pragma once
#include "mwrt_oe.hip.h"

namespace mwrt {
namespace sel {

constexpr int THREADS = oe::THREADS;   // one workgroup of four waves per profile
constexpr int WAVES = THREADS / 64;    // a wave per row of K: wave w owns the rows w, w + WAVES, ...
constexpr int ROWS_IN_FLIGHT = 4;      // ... and issues the loads of this many of them before it works on the first

struct SelArgs {
  const double* k0; const double* k1; const double* k2; const double* k3;   // K blocks [nprof][m][nlev]; unused ones null
  const double* s0;                         // [n][n] or [nprof][n][n] symmetric: the start covariance
  const double* se;                         // [m] or [nprof][m]: variances
  const double* sa_inv;                     // [n][n] symmetric or null (read for dfs_gain alone)
  const uint8_t* keep;                      // [nprof][m] or null
  const uint8_t* candidate;                 // [m] or null
  const uint8_t* active;                    // [nprof] or null: 0 skips the profile
  int32_t* order; double* q_pick;           // [nprof][nsel]
  int32_t* rank; double* q;                 // [nprof][m]; q is the work vector
  int32_t* count; uint8_t* status;          // [nprof]
  double* dfs_gain;                         // [nprof][nsel] or null
  double* post_cov; double* post_var;       // [nprof][n][n], [nprof][n] or null
  int nblk, nlev, m, n, nsel;
  int se_per_profile, s0_per_profile;
};

// Summation orders, the same for a row whatever its index, its batch-mates or the outputs asked for:
//   (S k)_c   = sum l = 0 .. n - 1 ascending of fma(S[c][l], k[l], .)            (the initial pass, v = S k_j of a round)
//   k^T S k   = the wave tree over lanes of  k[lane] (S k)[lane] (+ fma k[lane + 64] (S k)[lane + 64])
//   k^T v     = the wave tree over lanes of  k[lane] v[lane] (+ fma k[lane + 64] v[lane + 64]);  d = se_j + k_j^T v
//   v^T Sa^-1 v = the same tree over v[lane] w[lane], w_c = sum l ascending of fma(Sa^-1[l][c], v[l], .)
//   S[i][c]  <- fma(-(v_i / d), v_c, S[i][c])
//   q_i      <- max(0, q_i - (k_i^T v)^2 / (d se_i))
//   argmax   : a wave keeps the first strict maximum of its rows in ascending order; the four waves' bests are compared
//              in wave order, a later one winning only when it is greater, or equal at a lower index

// k_sel_select: packed S | v [np] | u = v / d [np] | k_j, then w = Sa^-1 v [np] | the waves' best q [WAVES] | their
// indices and candidate counts (int [2 WAVES]).  `np` = n rounded up to 2, `nte` = n (n + 1) / 2 rounded up to 2.
struct SelPlan {
  int np;
  size_t nte, s, v, u, kj, best, ints, total_bytes;
};
__host__ __device__ inline SelPlan sel_plan(int n) {
  SelPlan p{};
  p.np = (n + 1) & ~1;
  p.nte = ((size_t)n * (n + 1) / 2 + 1) & ~(size_t)1;
  p.s = 0;
  p.v = p.nte;
  p.u = p.v + p.np;
  p.kj = p.u + p.np;
  p.best = p.kj + p.np;
  p.ints = p.best + WAVES;
  p.total_bytes = sizeof(double) * (p.ints + WAVES);
  return p;
}
// the elements of a row one lane owns: lane and, from n = 65 on, lane + 64
__host__ __device__ inline int cols_per_lane(int n) { return (n + 63) / 64; }

// hipGetLastError() of the launch; hipErrorInvalidValue when n is beyond MWRT_OE_NFORM_MAX_N
hipError_t launch_select(const SelArgs& a, int64_t nprof, hipStream_t st);

}  // namespace sel
}  // namespace mwrt
