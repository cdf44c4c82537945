// mwrt_oe_lm.hip.h -- the Levenberg-Marquardt split of the optimal-estimation step (csrc/mwrt_oe_lm.hip):
// argument record, LDS plans and launchers only, as the host unit reads them.  No kernel lives here; the plans are host
// and device code so that launcher and kernel lay the block out by the same rule.
#pragma once
#include "mwrt_oe.hip.h"

namespace mwrt {
namespace lm {

constexpr int THREADS = oe::THREADS;   // one workgroup per profile, in all three kernels

// `o` holds the inputs of the step as k_oe_step reads them (K blocks, x, xa, Sa, Se, y, fx, the dimensions) and the trial
// outputs of the solve (x_new, status, chi2, nobs); dfs and post_var stay null.
struct LmArgs {
  oe::OeArgs o;
  const double* gamma;                      // [nprof]
  double* g0;                               // [nprof][m (m + 1) / 2] packed lower triangle of K Sa K^T
  double* r; double* kdx;                   // [nprof][m]  y - F(x) and K (x - xa), 0 in a dropped row
  uint8_t* keep;                            // [nprof][m]  1: the row is used
  uint8_t* lin_status;                      // [nprof]
  const uint8_t* active;                    // [nprof] or null: 0 skips the profile
  const double* sa_inv;                     // [n][n] symmetric (cost)
  double* cost; double* cost_obs; double* cost_prior;   // [nprof]; the last two may be null
};

// k_lm_prepare<MR> is steps 1-3 of k_oe_step and lays its block out by oe::lds_plan.

// k_lm_solve: packed G | d [mp] | u [mp] | v [n] | keep (int [mp]).  `mp` = m rounded up to 2.
struct SolvePlan {
  int mp;
  size_t g, d, u, v, keep, total_bytes;
};
__host__ __device__ inline SolvePlan solve_plan(int m, int n) {
  SolvePlan p{};
  p.mp = (m + 1) & ~1;
  p.g = 0;
  p.d = ((size_t)m * (m + 1) / 2 + 1) & ~(size_t)1;
  p.u = p.d + p.mp;
  p.v = p.u + p.mp;
  p.keep = p.v + (((size_t)n + 1) & ~(size_t)1);
  p.total_bytes = sizeof(double) * (p.keep + (size_t)p.mp / 2);
  return p;
}

// k_lm_cost: x - xa [n] | r [mp] | red [THREADS] | keep (int [mp]) | with a full Se, the packed kept sub-matrix
struct CostPlan {
  int mp;
  size_t dx, r, red, keep, s, total_bytes;
};
__host__ __device__ inline CostPlan cost_plan(int m, int n, int se_full) {
  CostPlan p{};
  p.mp = (m + 1) & ~1;
  p.dx = 0;
  p.r = ((size_t)n + 1) & ~(size_t)1;
  p.red = p.r + p.mp;
  p.keep = p.red + THREADS;
  p.s = p.keep + (size_t)p.mp / 2;
  p.total_bytes = sizeof(double) * (p.s + (se_full ? (((size_t)m * (m + 1) / 2 + 1) & ~(size_t)1) : 0));
  return p;
}

// hipGetLastError() of the launch; hipErrorInvalidValue when m is beyond MWRT_OE_MAX_M
hipError_t launch_lm_prepare(const LmArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_lm_solve(const LmArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_lm_cost(const LmArgs& a, int64_t nprof, hipStream_t st);

}  // namespace lm
}  // namespace mwrt
