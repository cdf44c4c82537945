// mwrt_nform.hip.h -- the n-form of the optimal-estimation step (csrc/mwrt_nform.hip): argument record, LDS
// plans and launchers only, as the host unit reads them.  No kernel lives here; the plans are host and device code so that
// launcher and kernel lay the block out by the same rule.
#pragma once
#include "mwrt_oe.hip.h"

namespace mwrt {
namespace nf {

constexpr int THREADS = oe::THREADS;   // one workgroup per profile, in all three kernels
constexpr int ROW_CHUNK = 16;          // rows of K staged in LDS at a time: four per wave, one wave per row
constexpr int TILE = 4;                // a thread owns TILE x TILE tiles of the packed lower triangle of H
constexpr int MAX_TILES = 3;           // ... at most three of them: 33 * 32 / 2 = 528 tiles at n = 128

struct NfArgs {
  const double* k0; const double* k1; const double* k2; const double* k3;   // K blocks [nprof][m][nlev]; unused ones null
  const double* x; const double* xa;        // [nprof][n]; xa [n] or [nprof][n]
  const double* sa_inv;                     // [n][n] symmetric
  const double* se;                         // [m] or [nprof][m]: variances
  const double* y; const double* fx;        // [nprof][m]
  const double* gamma;                      // [nprof] or null: 0
  const uint8_t* active;                    // [nprof] or null: 0 skips the profile
  double* h;                                // [nprof][n (n + 1) / 2] packed lower triangle of K^T W K
  double* g; double* rwr;                   // [nprof][n] K^T W r, [nprof] r^T W r
  uint8_t* keep; int32_t* nobs;             // [nprof][m], [nprof]
  uint8_t* lin_status;                      // [nprof]
  double* x_new; uint8_t* status;           // [nprof][n], [nprof]
  double* chi2; double* dfs;                // [nprof] or null
  double* post_var; double* post_cov;       // [nprof][n], [nprof][n][n] or null
  double* cost; double* cost_obs; double* cost_prior;   // [nprof]; the last two may be null
  int nblk, nlev, m, n;
  int xa_per_profile, se_per_profile;
};

// tiles of the lower triangle of H and how many of them a thread owns
__host__ __device__ inline int tile_count(int n) {
  const int nb = (n + TILE - 1) / TILE;
  return nb * (nb + 1) / 2;
}
__host__ __device__ inline int tiles_per_thread(int n) { return (tile_count(n) + THREADS - 1) / THREADS; }

// k_nf_normal<TT>: Ks [ROW_CHUNK][pitch] the rows kept, else 0 | Kw [ROW_CHUNK][pitch] the same times 1 / se_i |
// res [ROW_CHUNK] y - F | wres [ROW_CHUNK] (y - F) / se | counts (int [8]: rows kept and bad variances per wave).
// `pitch` = n rounded up to TILE: the columns n .. pitch - 1 are staged as 0.
struct NormalPlan {
  int pitch;
  size_t ks, kw, res, wres, counts, total_bytes;
};
__host__ __device__ inline NormalPlan normal_plan(int n) {
  NormalPlan p{};
  p.pitch = ((n + TILE - 1) / TILE) * TILE;
  p.ks = 0;
  p.kw = (size_t)ROW_CHUNK * p.pitch;
  p.res = 2 * (size_t)ROW_CHUNK * p.pitch;
  p.wres = p.res + ROW_CHUNK;
  p.counts = p.wres + ROW_CHUNK;
  p.total_bytes = sizeof(double) * (p.counts + 4);
  return p;
}

// k_nf_solve: packed C, then L, then L^-1 | rhs [np] | s [np] | x - xa [np] | x+ - xa [np] | red [THREADS].
// `np` = n rounded up to 2.
struct SolvePlan {
  int np;
  size_t c, rhs, s, dx, de, red, total_bytes;
};
__host__ __device__ inline SolvePlan solve_plan(int n) {
  SolvePlan p{};
  p.np = (n + 1) & ~1;
  p.c = 0;
  p.rhs = ((size_t)n * (n + 1) / 2 + 1) & ~(size_t)1;
  p.s = p.rhs + p.np;
  p.dx = p.s + p.np;
  p.de = p.dx + p.np;
  p.red = p.de + p.np;
  p.total_bytes = sizeof(double) * (p.red + THREADS);
  return p;
}

// k_nf_cost: x - xa [np] | red [THREADS]
struct CostPlan {
  size_t dx, red, total_bytes;
};
__host__ __device__ inline CostPlan cost_plan(int n) {
  CostPlan p{};
  p.dx = 0;
  p.red = ((size_t)n + 1) & ~(size_t)1;
  p.total_bytes = sizeof(double) * (p.red + THREADS);
  return p;
}

// hipGetLastError() of the launch; hipErrorInvalidValue when n is beyond MWRT_OE_NFORM_MAX_N
hipError_t launch_nf_normal(const NfArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_nf_solve(const NfArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_nf_cost(const NfArgs& a, int64_t nprof, hipStream_t st);

}  // namespace nf
}  // namespace mwrt
