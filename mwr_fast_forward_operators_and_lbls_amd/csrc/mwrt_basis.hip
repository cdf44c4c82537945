// mwrt_basis.hip -- the reduced-basis state map (include/mwrt.h mwrt_basis_project_device / mwrt_basis_expand_device,
// DESIGN 4.9).  With x = x_ref + B c the 1D-Var update needs K B instead of K:
//     K_c[p][i][j] = sum over b < nblk, l < nlev of K_b[p][i][l] * B[b nlev + l][j]                      (k_project)
//     x[p][k]      = x_ref[k] + sum over j < r of B[k][j] * c[p][j]                                       (k_expand)
//   k_project   B is shared by the batch, so the nprof * m rows are one tall, thin product.  A workgroup owns ROWS = 128
//               rows and COLS = 32 columns; the contraction runs in chunks of KCHUNK = 16 staged in LDS (K transposed into
//               Ks [KCHUNK][KPITCH], B into Bs [KCHUNK][COLS]) with the next chunk's global loads in flight while this one
//               is contracted, as form_panel of mwrt_oe_blocks.hip.h does.  A thread keeps a 4 x 4 register tile of plain
//               fp64 FMAs: per contraction index 4 + 4 LDS doubles feed 16 FMAs.  Columns beyond one tile are blockIdx.y.
//   k_expand    one thread per element of x; small and not hot.
// No atomics, no workspace, no scratch.  Every output element is one FMA chain in the order mwrt_basis.hip.h states, fed by
// its own K row (its own c) and B alone: the same bit for bit whatever nprof, the rows that share its tile, the other
// columns asked for, or the call.  A non-finite K element reaches its own output row and no other; a row of zeros gives
// exactly 0.0.  Every global index is 64-bit.
#include "mwrt_basis.hip.h"

namespace mwrt {
namespace basis {

namespace {

// one contraction chunk on its way from global memory to LDS: 2 MR K elements and two B elements per thread
struct Chunk {
  double k[2 * MR], s[2];
  __device__ __forceinline__ void fetch(const ProjectArgs& A, int64_t row0, int k0, int j0, int tid) {
    const int lkk = tid & (KCHUNK - 1), li = tid / KCHUNK;
    const int kk = k0 + lkk;
    const bool kin = kk < A.n;
    const int b = kin ? kk / A.nlev : 0;
    const int l = kin ? kk - b * A.nlev : 0;
    const double* base = (b == 0 ? A.in0 : b == 1 ? A.in1 : b == 2 ? A.in2 : A.in3) + l;
#pragma unroll
    for (int q = 0; q < 2 * MR; ++q) {
      const int64_t row = row0 + li + (THREADS / KCHUNK) * q;
      k[q] = (kin && row < A.nrows) ? base[row * A.nlev] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + THREADS * q;
      const int kr = k0 + e / COLS, jc = j0 + (e & (COLS - 1));
      s[q] = (kr < A.n && jc < A.r) ? A.b[(int64_t)kr * A.r + jc] : 0.0;
    }
  }
  __device__ __forceinline__ void store(double* Ks, double* Bs, int tid) const {
    const int lkk = tid & (KCHUNK - 1), li = tid / KCHUNK;
#pragma unroll
    for (int q = 0; q < 2 * MR; ++q) Ks[lkk * KPITCH + li + (THREADS / KCHUNK) * q] = k[q];
#pragma unroll
    for (int q = 0; q < 2; ++q) Bs[tid + THREADS * q] = s[q];
  }
};

__global__ void __launch_bounds__(THREADS)
k_project(const ProjectArgs A) {
  __shared__ double Ks[KCHUNK * KPITCH];
  __shared__ double Bs[KCHUNK * COLS];
  const int tid = threadIdx.x;
  const int ti = tid >> 3, tj = tid & 7;
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  const int j0 = (int)blockIdx.y * COLS;
  double acc[MR][NC];
#pragma unroll
  for (int q = 0; q < MR; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[q][c] = 0.0;
  Chunk ch;
  ch.fetch(A, row0, 0, j0, tid);
  for (int k0 = 0; k0 < A.n; k0 += KCHUNK) {
    ch.store(Ks, Bs, tid);
    __syncthreads();
    if (k0 + KCHUNK < A.n) ch.fetch(A, row0, k0 + KCHUNK, j0, tid);   // in flight while this chunk is contracted
#pragma unroll
    for (int kk = 0; kk < KCHUNK; ++kk) {
      double a[MR], s[NC];
#pragma unroll
      for (int q = 0; q < MR; ++q) a[q] = Ks[kk * KPITCH + ti + (THREADS / 8) * q];
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = Bs[kk * COLS + tj * NC + c];
#pragma unroll
      for (int q = 0; q < MR; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[q][c] = fma(a[q], s[c], acc[q][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < MR; ++q) {
    const int64_t row = row0 + ti + (THREADS / 8) * q;
    if (row >= A.nrows) continue;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = j0 + tj * NC + c;
      if (j < A.r) A.out[row * A.r + j] = acc[q][c];
    }
  }
}

__global__ void __launch_bounds__(THREADS)
k_expand(const ExpandArgs A) {
  const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e >= A.total) return;
  const int64_t p = e / A.n;
  const int64_t k = e - p * A.n;
  const double* b = A.b + k * A.r;
  const double* c = A.c + p * A.r;
  double acc = A.x_ref[A.per_profile ? e : k];
  for (int j = 0; j < A.r; ++j) acc = fma(b[j], c[j], acc);
  A.x[e] = acc;
}

}  // namespace

hipError_t launch_project(const ProjectArgs& a, hipStream_t st) {
  const int64_t bx = (a.nrows + ROWS - 1) / ROWS;
  const int64_t by = ((int64_t)a.r + COLS - 1) / COLS;
  if (bx < 1 || by < 1 || by > 65535 || bx * by > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_project, dim3((unsigned)bx, (unsigned)by), dim3(THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_expand(const ExpandArgs& a, hipStream_t st) {
  const int64_t blocks = (a.total + THREADS - 1) / THREADS;
  if (blocks < 1 || blocks > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_expand, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace basis
}  // namespace mwrt
