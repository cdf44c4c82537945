// mwrt_basis.hip.h -- the reduced-basis state map (csrc/mwrt_basis.hip): the tiling plan, the argument
// records and the launchers only, as the host unit reads them.  No kernel lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mwrt {
namespace basis {

// k_project: one workgroup per (ROWS rows of the batch, COLS columns of the basis); grid = (row tiles, column tiles)
constexpr int THREADS = 256;               // four waves per workgroup
constexpr int ROWS = 128;                  // rows (profile, observation) of a workgroup's tile
constexpr int COLS = 32;                   // basis columns of a workgroup's tile
constexpr int KCHUNK = 16;                 // contraction indices staged in LDS at a time
constexpr int MR = 4;                      // register tile: a thread owns rows ti + 32 q, q < MR ...
constexpr int NC = 4;                      // ... and columns 4 tj + c, c < NC;  (THREADS / 8) * MR = ROWS, 8 * NC = COLS
constexpr int KPITCH = ROWS + 1;           // odd pitch of Ks [KCHUNK][KPITCH]: the transposed stores spread over the banks
static_assert((THREADS / 8) * MR == ROWS && 8 * NC == COLS && THREADS / KCHUNK * 2 * MR == ROWS, "tile plan");
static_assert(THREADS * 2 == KCHUNK * COLS, "a thread stages two elements of a B chunk");

// Summation order of k_project, the same for every element whatever the tile it falls in:
//   acc = 0.0;  for b = 0 .. nblk - 1, for l = 0 .. nlev - 1 (b outer, l ascending):  acc = fma(K_b[row][l], B[b nlev + l][j], acc)
// The last chunk is padded with fma(0.0, 0.0, acc), which leaves acc as it is bit for bit (acc is never -0.0).
struct ProjectArgs {
  const double* in0; const double* in1; const double* in2; const double* in3;   // [nrows][nlev], nrows = nprof * m
  const double* b;                          // [nblk * nlev][r]
  double* out;                              // [nrows][r]
  int64_t nrows;
  int32_t nlev, nblk, n, r;                 // n = nblk * nlev
};

// k_expand: one thread per element of x [nprof][n]
//   acc = x_ref[k] (or x_ref[p][k]);  for j = 0 .. r - 1 ascending:  acc = fma(B[k][j], c[p][j], acc);  x[p][k] = acc
struct ExpandArgs {
  const double* b;                          // [n][r]
  const double* c;                          // [nprof][r]
  const double* x_ref;                      // [n], or [nprof][n] with per_profile
  double* x;                                // [nprof][n]
  int64_t total;                            // nprof * n
  int32_t n, r, per_profile;
};

// hipGetLastError() of the launch; hipErrorInvalidValue when the grid would exceed 2^31 - 1 workgroups
hipError_t launch_project(const ProjectArgs& a, hipStream_t st);
hipError_t launch_expand(const ExpandArgs& a, hipStream_t st);

}  // namespace basis
}  // namespace mwrt
