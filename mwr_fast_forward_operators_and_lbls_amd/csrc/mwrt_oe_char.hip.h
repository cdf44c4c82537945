// mwrt_oe_char.hip.h -- the characterisation of the optimal-estimation step (csrc/mwrt_oe_char.hip): argument
// records, LDS plan and launchers only, as the host unit reads them.  No kernel lives here; the plan is host and device
// code so that launcher and kernel lay the block out by the same rule.
#pragma once
#include "mwrt_oe.hip.h"

namespace mwrt {
namespace oec {

constexpr int THREADS = oe::THREADS;   // one workgroup per profile (gain) or per output tile (product)
constexpr int TILE = 64;               // k_char_product: a workgroup's square tile of the n x n result
constexpr int PCHUNK = 16;             // k_char_product: observation rows staged in LDS at a time
constexpr int PARTS = THREADS / oe::PANEL;   // 8 threads share one column of a panel in the column sums

// `o` holds the inputs of the step as k_oe_step reads them (K blocks, x, xa, Sa, Se, y, fx, the dimensions) and status and
// nobs; x_new, chi2, dfs and post_var stay null.
struct GainArgs {
  oe::OeArgs o;
  double* gain; double* ksa;                // [nprof][m][n] or null
  uint8_t* keep;                            // [nprof][m] or null
  double* avk_diag; double* noise_var; double* smooth_var;   // [nprof][n] or null
  double* dfs_block;                        // [nprof][nblk] or null
};

// k_char_gain<MR>: packed G (then L, then L^-1) | Wt [PANEL][kpitch] (W_p, then Z_p, then gain^T_p) | Ks [KCHUNK][kpitch] |
// Ss [KCHUNK][PANEL] (Ks and Ss hold the column sums of Z^2 after the panel is formed) | part [2][PARTS][PANEL] |
// sed [mp] | red [THREADS] | keep (int [mp]).  In doubles from the start of the block; every offset is even (16 bytes).
// Nothing depends on n: 149.4 KiB at m = 140, whatever n is.
struct GainPlan {
  int mp, kpitch;
  size_t g, wt, ks, ss, part, sed, red, keep, total_bytes;
};
__host__ __device__ inline GainPlan gain_plan(int m) {
  GainPlan p{};
  p.mp = ((m + oe::ROW_TILE - 1) / oe::ROW_TILE) * oe::ROW_TILE;
  p.kpitch = p.mp + 1;
  p.g = 0;
  p.wt = ((size_t)m * (m + 1) / 2 + 1) & ~(size_t)1;
  p.ks = p.wt + (((size_t)oe::PANEL * p.kpitch + 1) & ~(size_t)1);
  p.ss = p.ks + (size_t)oe::KCHUNK * p.kpitch;              // contiguous with Ks: together >= ROW_TILE * PANEL doubles
  p.part = (p.ss + (size_t)oe::KCHUNK * oe::PANEL + 1) & ~(size_t)1;
  p.sed = p.part + (size_t)2 * PARTS * oe::PANEL;
  p.red = p.sed + p.mp;
  p.keep = p.red + THREADS;
  p.total_bytes = sizeof(double) * (p.keep + (size_t)p.mp / 2);
  return p;
}

// C[p] = L[p]^T R[p] over the rows kept, rows [row_begin, row_begin + rows) of the n x n result; both operands [m][.]
// row-major.  The right operand is nrb arrays of [nprof][m][rcols] side by side (K: nblk of nlev; W: one of n).
struct ProductArgs {
  const double* left;                       // gain [nprof][m][n]
  const double* r0; const double* r1; const double* r2; const double* r3;
  const uint8_t* keep;                      // [nprof][m]
  const double* sa;                         // [n][n]: out = Sa - C; null: out = C
  double* out;                              // [nprof][rows][n]
  int m, n, rcols;
  int row_begin, rows;
  int tiles_x, tiles_y;
};
constexpr size_t PRODUCT_LDS_BYTES = sizeof(double) * 2 * PCHUNK * TILE;   // Ls | Rs, [PCHUNK][TILE] each

// hipGetLastError() of the launch; hipErrorInvalidValue when m is beyond MWRT_OE_MAX_M or the grid beyond 2^31 - 1
hipError_t launch_char_gain(const GainArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_char_product(const ProductArgs& a, int64_t nprof, hipStream_t st);

}  // namespace oec
}  // namespace mwrt
