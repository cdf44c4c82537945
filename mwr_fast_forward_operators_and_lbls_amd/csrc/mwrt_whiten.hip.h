// mwrt_whiten.hip.h -- pre-whitening with a per-profile observation-error covariance (csrc/mwrt_whiten.hip):
// the plan, the argument records and the launchers only, as the host unit reads them.  No kernel lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mwrt {
namespace wh {

// k_wh_factor: one workgroup of FACTOR_THREADS per profile (the row rule with one wave per row, the kept Se_p as a packed
// lower triangle in LDS, cholesky_packed of mwrt_oe_blocks.hip.h).
// k_wh_apply: one workgroup of one wave per (profile, column tile); a lane owns one column of the tile, which lives in
// LDS as vt [m][COLS] and is solved in place, ROW_BLOCK rows abreast with the rows beyond the last full block one by one.
constexpr int FACTOR_THREADS = 256;        // = oe::THREADS: the blocks of mwrt_oe_blocks.hip.h are written for it
constexpr int COLS = 64;                   // columns (levels) of a tile: one per lane, so K is read and written coalesced
constexpr int ROW_BLOCK = 4;               // rows solved abreast: one LDS read of a solved row feeds ROW_BLOCK FMA chains
constexpr int LOAD_BATCH = 14;             // rows of the tile whose global loads are in flight together (98 = 7 * 14, 140 = 10 * 14)
constexpr int STAGE_MAX = ROW_BLOCK * 140 + ROW_BLOCK * (ROW_BLOCK + 1) / 2;   // doubles of L a block of rows needs at m = 140
constexpr int STAGE_REGS = (STAGE_MAX + COLS - 1) / COLS;                     // ... per lane while they are fetched ahead: 9
constexpr int KEEP_WORDS = 3;              // the row flags of a profile as 64-bit masks in SGPRs: m <= 192

// Dynamic LDS in bytes.  The factorisation passes 64 KiB at m = 127 | 128, the tile with its stage of L at 120 | 121, where
// the launchers raise the limit.
__host__ __device__ inline size_t factor_lds_bytes(int m) {
  return sizeof(double) * ((((size_t)m * (m + 1) / 2 + 1) & ~(size_t)1) + ((size_t)m + 1) / 2);   // G, then int keep[m]
}
__host__ __device__ inline size_t apply_lds_bytes(int m) {      // vt [m][COLS], then the rows of L of one block of rows
  return sizeof(double) * ((size_t)m * COLS + (size_t)ROW_BLOCK * m + ROW_BLOCK * (ROW_BLOCK + 1) / 2);
}

// Row i of profile p is kept when y, F, every K_b[p][i][:] and its Se entry (the variance, or every element of row i of a
// full Se_p) are finite.  G = Se_p on the kept rows and columns (lower triangle as stored), a dropped row a row of the
// identity; L = cholesky_packed(G).  status 1: ok; 2: a pivot fails pivot > 0 (L all NaN, keep 0); 3: no row kept (L = I).
struct FactorArgs {
  const double* k0; const double* k1; const double* k2; const double* k3;   // [nprof][m][nlev]; unused ones null
  const double* se;                         // [nprof][m] or [nprof][m][m]
  const double* y; const double* fx;        // [nprof][m]
  double* l;                                // [nprof][m (m + 1) / 2]
  uint8_t* keep;                            // [nprof][m]
  uint8_t* status;                          // [nprof]
  int32_t nblk, nlev, m, se_full;
};

// Per column v of a block or a vector, with the rows that keep[] drops read as 0 (loaded first, selected afterwards):
//   mode 0:  i ascending:   acc = v_i;  for j = 0 .. i - 1 ascending:       acc = fma(-L_ij, w_j, acc);  w_i = acc / L_ii
//   mode 1:  i descending:  acc = v_i;  for j = m - 1 .. i + 1 descending:  acc = fma(-L_ji, w_j, acc);  w_i = acc / L_ii
//            (carried out row j by row j: once w_j is known it is taken off every acc_i, i < j -- the same FMAs in the same order)
// A dropped row takes part with L_ij = 0 and w_j = 0, which leaves acc as it is bit for bit; its output is 0.0 in a block and
// NaN in a vector.  A profile whose L[0] is NaN (status 2 of the factorisation) gets NaN in every output.
struct ApplyArgs {
  const double* in0; const double* in1; const double* in2; const double* in3;   // [nprof][m][nlev]
  double* out0; double* out1; double* out2; double* out3;
  const double* v_in0; const double* v_in1;                                      // [nprof][m], either may be null
  double* v_out0; double* v_out1;
  const double* l;                          // [nprof][m (m + 1) / 2]
  const uint8_t* keep;                      // [nprof][m]
  int32_t nblk, nlev, m, mode;
  int32_t ctiles;                           // column tiles of a block: ceil(nlev / COLS)
  int32_t tiles;                            // tiles of a profile: nblk * ctiles, and one more for the vectors (lanes 0 and 1)
};

// hipGetLastError() of the launch (or the error of raising the LDS limit); hipErrorInvalidValue beyond 2^31 - 1 workgroups
hipError_t launch_factor(const FactorArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_apply(const ApplyArgs& a, int64_t nprof, hipStream_t st);

}  // namespace wh
}  // namespace mwrt
