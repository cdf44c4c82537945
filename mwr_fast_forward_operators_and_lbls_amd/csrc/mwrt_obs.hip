// mwrt_obs.hip -- the instrument operator (include/mwrt.h mwrt_obs_apply_device): channel quantities from
// monochromatic pencil-beam ones on a quadrature grid, a fixed sparse linear map in CSR form applied along the rows of
// the brightness temperatures ([nprof][m_in], nlev = 1) and of up to four K-matrix blocks ([nprof][m_in][nlev]):
//     out[p][o][l] = sum over e in [row_ptr[o], row_ptr[o + 1]) of w[e] * in[p][col[e]][l]
//   k_obs_apply   one wave per (profile, block, output row, chunk of 64 levels); four such items per workgroup, so at
//                 nlev = 180 a workgroup spans more than one output row.  The lanes of a wave are consecutive levels:
//                 every load and store is one coalesced run of doubles.  The item -- and with it the row's (col, w) pairs
//                 -- is the same in every lane (scalar loads); the non-zero loop is unrolled 8, 4, 2, 1 so that up to
//                 eight row loads are in flight per lane before the first FMA.
// A pure streaming reduction: no LDS, no atomics, no workspace.  The sum is FMA-accumulated from 0.0 in the stored order
// of the row, whatever the unroll step, so an element is the same bit for bit whatever nprof, the blocks asked for or the
// call it is computed in; an empty row is exactly 0.0; a NaN or Inf input reaches only the rows that reference it (an
// explicit zero weight on it included: 0 * NaN = NaN, IEEE).  Every index is 64-bit.
#include "mwrt_obs.hip.h"

namespace mwrt {
namespace obs {

namespace {

// U entries of the row from e on: the loads first, then the FMAs in the stored order
template <int U>
__device__ __forceinline__ double accumulate(const ObsArgs& A, const double* in, int64_t nlev, int e, double acc) {
  double v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = in[(int64_t)A.col[e + u] * nlev];
#pragma unroll
  for (int u = 0; u < U; ++u) acc = fma(A.w[e + u], v[u], acc);
  return acc;
}

__global__ void __launch_bounds__(THREADS)
k_obs_apply(const ObsArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int64_t item = (int64_t)blockIdx.x * ITEMS + wave;
  if (item >= A.items) return;                             // the same in every lane of the wave
  const int64_t row = item / A.nchunks;                    // (prof * nblk + b) * m_out + o
  const int chunk = (int)(item - row * A.nchunks);
  const int64_t pb = row / A.m_out;
  const int o = (int)(row - pb * A.m_out);
  const int64_t prof = pb / A.nblk;
  const int b = (int)(pb - prof * A.nblk);
  const int l = chunk * WAVE + lane;
  if (l >= A.nlev) return;
  const int64_t nlev = A.nlev;
  const double* in = (b == 0 ? A.in0 : b == 1 ? A.in1 : b == 2 ? A.in2 : A.in3) + prof * A.m_in * nlev + l;
  double* out = (b == 0 ? A.out0 : b == 1 ? A.out1 : b == 2 ? A.out2 : A.out3) + (prof * A.m_out + o) * nlev + l;
  int e = A.row_ptr[o];
  const int e1 = A.row_ptr[o + 1];
  double acc = 0.0;
  for (; e + UNROLL <= e1; e += UNROLL) acc = accumulate<UNROLL>(A, in, nlev, e, acc);
  if (e + 4 <= e1) { acc = accumulate<4>(A, in, nlev, e, acc); e += 4; }
  if (e + 2 <= e1) { acc = accumulate<2>(A, in, nlev, e, acc); e += 2; }
  if (e < e1) acc = accumulate<1>(A, in, nlev, e, acc);
  *out = acc;
}

}  // namespace

hipError_t launch_obs_apply(const ObsArgs& a, hipStream_t st) {
  const int64_t blocks = (a.items + ITEMS - 1) / ITEMS;
  if (blocks < 1 || blocks > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_obs_apply, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace obs
}  // namespace mwrt
