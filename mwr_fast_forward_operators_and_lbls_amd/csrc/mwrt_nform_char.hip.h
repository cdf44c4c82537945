// mwrt_nform_char.hip.h -- the characterisation of the n-form step (csrc/mwrt_nform_char.hip): argument
// record, the LDS plan, the tiling of the gain and the launchers only, as the host unit reads them.  No kernel lives here;
// the plan is host and device code so that launcher and kernel lay the block out by the same rule.
#pragma once
#include "mwrt_oe.hip.h"

namespace mwrt {
namespace nfc {

constexpr int THREADS = oe::THREADS;   // four waves per workgroup in both kernels
// k_nfc_gain: one workgroup per (profile, ROWS observation rows, COLS state columns), the tile plan of k_project
constexpr int ROWS = 128;              // rows of a workgroup's tile; a tile never leaves its profile
constexpr int COLS = 32;               // columns of a workgroup's tile
constexpr int KCHUNK = 16;             // contraction indices staged in LDS at a time
constexpr int MR = 4;                  // register tile: a thread owns rows ti + 32 q, q < MR ...
constexpr int NC = 4;                  // ... and columns 4 tj + c, c < NC
constexpr int KPITCH = ROWS + 1;       // odd pitch of Ks [KCHUNK][KPITCH]: the transposed stores spread over the banks
static_assert((THREADS / 8) * MR == ROWS && 8 * NC == COLS && THREADS / KCHUNK * 2 * MR == ROWS, "tile plan");
static_assert(THREADS * 2 == KCHUNK * COLS, "a thread stages two elements of a chunk of S^");

struct CharArgs {
  const double* k0; const double* k1; const double* k2; const double* k3;   // K blocks [nprof][m][nlev]; unused ones null (gain)
  const double* sa_inv;                     // [n][n] symmetric                                   (char)
  const double* se;                         // [m] or [nprof][m]: variances                       (gain)
  const double* h;                          // [nprof][n (n + 1) / 2] packed K^T W K              (char)
  const uint8_t* lin_status;                // [nprof]                                            (char)
  const uint8_t* keep;                      // [nprof][m]                                         (gain)
  const uint8_t* active;                    // [nprof] or null: 0 skips the profile
  uint8_t* status;                          // [nprof]: written by char, read by gain
  double* post_cov;                         // [nprof][n][n]: written by char (or null), read by gain
  double* avk;                              // [nprof][rows][n] or null
  double* avk_diag; double* noise_var; double* smooth_var;   // [nprof][n] or null
  double* dfs_block;                        // [nprof][nblk] or null
  double* gain;                             // [nprof][m][n]
  int nblk, nlev, m, n;
  int se_per_profile, row_begin, rows;      // rows: the count itself, n for "all"
};

// Summation orders, the same for an element whatever the window, the tile or the outputs asked for:
//   S^[i][j]   = sum k = max(i, j) .. n - 1 ascending of fma(X[k][i], X[k][j], .), X = L^-1      (as k_nf_solve)
//   A[i][j]    = sum l = 0 .. n - 1 ascending of fma(S^[i][l], H[l][j], .)
//   noise[j]   = wave tree over lanes of  A[j][lane] S^[lane][j] (+ fma A[j][lane + 64] S^[lane + 64][j])
//   dfs_block  = the block tree (oe::block_sum) over thread t's A[t][t] when t lies in the block, else 0.0
//   gain[i][j] = sum k = 0 .. n - 1 ascending of fma(keep_i ? K[i][k] * (1 / se_i) : 0, S^[k][j], .); the last chunk is
//                padded with fma(0.0, 0.0, acc)

// k_nfc_char: packed C, then L, then L^-1, at last packed H | packed S^ | diag A [np] | red [THREADS].  `np` = n rounded
// up to 2, `nte` = n (n + 1) / 2 rounded up to 2.
struct CharPlan {
  int np;
  size_t nte, c, s, dg, red, total_bytes;
};
__host__ __device__ inline CharPlan char_plan(int n) {
  CharPlan p{};
  p.np = (n + 1) & ~1;
  p.nte = ((size_t)n * (n + 1) / 2 + 1) & ~(size_t)1;
  p.c = 0;
  p.s = p.nte;
  p.dg = 2 * p.nte;
  p.red = p.dg + p.np;
  p.total_bytes = sizeof(double) * (p.red + THREADS);
  return p;
}
// the columns of a row of A one lane owns: lane and, from n = 65 on, lane + 64
__host__ __device__ inline int cols_per_lane(int n) { return (n + 63) / 64; }

// row tiles of one profile and column tiles of the gain
__host__ __device__ inline int64_t gain_row_tiles(int m) { return ((int64_t)m + ROWS - 1) / ROWS; }
__host__ __device__ inline int gain_col_tiles(int n) { return (n + COLS - 1) / COLS; }

// hipGetLastError() of the launch; hipErrorInvalidValue when n is beyond MWRT_OE_NFORM_MAX_N or the grid beyond 2^31 - 1
hipError_t launch_nfc_char(const CharArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_nfc_gain(const CharArgs& a, int64_t nprof, hipStream_t st);

}  // namespace nfc
}  // namespace mwrt
