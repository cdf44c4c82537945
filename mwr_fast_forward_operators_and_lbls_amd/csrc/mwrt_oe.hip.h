// mwrt_oe.hip.h -- the optimal-estimation step (csrc/mwrt_oe.hip): argument record, LDS plan and launcher
// only, as the host unit reads them.  No kernel lives here; lds_plan is host and device code so that the launcher and the
// kernel lay the block out by the same rule (the host unit uses its host side alone).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/mwrt.h"

namespace mwrt {
namespace oe {

constexpr int THREADS = 256;       // one workgroup per profile
constexpr int PANEL = 32;          // columns of Sa per panel of W = K Sa
constexpr int KCHUNK = 16;         // contraction indices staged in LDS at a time
constexpr int ROW_TILE = 32;       // observation rows per register-tile step: a thread owns rows ti, ti + 32, ...
constexpr int MAX_ROW_TILES = (MWRT_OE_MAX_M + ROW_TILE - 1) / ROW_TILE;   // 5

struct OeArgs {
  const double* k0; const double* k1; const double* k2; const double* k3;   // K blocks [nprof][m][nlev]; unused ones null
  const double* x; const double* xa;        // [nprof][n]; xa [n] or [nprof][n]
  const double* sa;                         // [n][n] symmetric
  const double* se;                         // [m] or [m][m]
  const double* y; const double* fx;        // [nprof][m]
  double* x_new;                            // [nprof][n]
  double* chi2; double* dfs;                // [nprof] or null
  double* post_var;                         // [nprof][n] or null
  int32_t* nobs;                            // [nprof] or null
  uint8_t* status;                          // [nprof]
  int nblk, nlev, m, n;
  int xa_per_profile, se_full;
};

// Dynamic LDS of one workgroup, in doubles from the start of the block.  `mp` = m rounded up to ROW_TILE.
struct LdsPlan {
  int mp, kpitch;
  size_t g, region, ks, ss, d, u, sed, red, keep, total_bytes;
};
__host__ __device__ inline LdsPlan lds_plan(int m, int n) {
  LdsPlan p{};
  p.mp = ((m + ROW_TILE - 1) / ROW_TILE) * ROW_TILE;
  p.kpitch = p.mp + 1;                                       // odd pitch: the transposed stores spread over the banks
  size_t g = ((size_t)m * (m + 1) / 2 + 1) & ~(size_t)1;     // packed lower triangle of G, then L, then L^-1
  p.g = 0;
  p.region = g;                                              // Wt [PANEL][kpitch] | Ks [KCHUNK][kpitch] | Ss [KCHUNK][PANEL];
  p.ks = p.region + (size_t)PANEL * p.kpitch;                //   the same doubles hold x - xa and later v = K^T u ([n])
  p.ss = p.ks + (size_t)KCHUNK * p.kpitch;
  size_t rlen = (size_t)(PANEL + KCHUNK) * p.kpitch + (size_t)KCHUNK * PANEL;
  if (rlen < (size_t)n) rlen = (size_t)n;
  rlen = (rlen + 1) & ~(size_t)1;
  p.d = p.region + rlen;
  p.u = p.d + p.mp;
  p.sed = p.u + p.mp;
  p.red = p.sed + p.mp;
  p.keep = p.red + THREADS;                                  // int [mp]
  p.total_bytes = sizeof(double) * (p.keep + (size_t)p.mp / 2);
  return p;
}

// hipGetLastError() of the launch; hipErrorInvalidValue when m is beyond MWRT_OE_MAX_M
hipError_t launch_oe_step(const OeArgs& a, int64_t nprof, hipStream_t st);

}  // namespace oe
}  // namespace mwrt
