// mwrt_oe_blocks.hip.h -- the device building blocks the optimal-estimation kernel units share (csrc/mwrt_oe.hip and
// csrc/mwrt_oe_lm.hip): finiteness, the packed-triangle index, the K-block row base, the wave and
// block sums, the register chunk of K and Sa, and the panel W_p = K Sa[:, panel].  Device code only: the host unit never
// includes this file.  Everything is force-inlined and sits in an unnamed namespace, so each unit gets its own copy.
#pragma once
#include "mwrt_oe.hip.h"

#include <math.h>

namespace mwrt {
namespace oe {

namespace {

__device__ __forceinline__ bool finite_f64(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, j <= i

// row base of K block b of this profile: entry [i][l] is at base[i * nlev + l]
__device__ __forceinline__ const double* kblock(const OeArgs& A, int b, int64_t prof) {
  const double* p = b == 0 ? A.k0 : b == 1 ? A.k1 : b == 2 ? A.k2 : A.k3;
  return p + (size_t)prof * A.m * A.nlev;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum of one value per thread in a fixed tree; every thread gets the result.  `red` is left free for the next use.
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// one chunk of KCHUNK contraction indices in registers: K[:, k0 .. k0 + 16) (rows li + 16 r) and, with SA,
// Sa[k0 .. k0 + 16)[j0 .. j0 + 32)
template <int MR, bool SA>
struct Chunk {
  double k[2 * MR];
  double s[2];
  __device__ __forceinline__ void fetch(const OeArgs& A, int64_t prof, const int* keep, int k0, int j0, int tid) {
    const int lkk = tid & (KCHUNK - 1), li = tid >> 4;
    const int kk = k0 + lkk;
    const bool kin = kk < A.n;
    const int b = kin ? kk / A.nlev : 0;
    const double* base = kblock(A, b, prof) + (kin ? kk - b * A.nlev : 0);
#pragma unroll
    for (int r = 0; r < 2 * MR; ++r) {
      const int i = li + 16 * r;
      const bool live = kin && i < A.m && keep[i] != 0;
      k[r] = live ? base[(size_t)i * A.nlev] : 0.0;
    }
    if (SA) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int e = tid + THREADS * q;
        const int kr = k0 + (e >> 5), jc = j0 + (e & (PANEL - 1));
        s[q] = (kr < A.n && jc < A.n) ? A.sa[(size_t)kr * A.n + jc] : 0.0;
      }
    }
  }
  __device__ __forceinline__ void store(double* Ks, double* Ss, int kpitch, int tid) const {
    const int lkk = tid & (KCHUNK - 1), li = tid >> 4;
#pragma unroll
    for (int r = 0; r < 2 * MR; ++r) Ks[lkk * kpitch + li + 16 * r] = k[r];
    if (SA) {
#pragma unroll
      for (int q = 0; q < 2; ++q) Ss[tid + THREADS * q] = s[q];
    }
  }
};

// W_p = K Sa[:, j0 .. j0 + 32) into Wt [PANEL][kpitch] (transposed: Wt[jj][i]).  Ends behind a barrier.
template <int MR>
__device__ __forceinline__ void form_panel(const OeArgs& A, int64_t prof, const int* keep, int j0, double* Wt, double* Ks,
                                           double* Ss, int kpitch, int tid) {
  const int ti = tid >> 3, tj = tid & 7;
  double acc[MR][4];
#pragma unroll
  for (int r = 0; r < MR; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  Chunk<MR, true> ch;
  ch.fetch(A, prof, keep, 0, j0, tid);
  for (int k0 = 0; k0 < A.n; k0 += KCHUNK) {
    ch.store(Ks, Ss, kpitch, tid);
    __syncthreads();
    if (k0 + KCHUNK < A.n) ch.fetch(A, prof, keep, k0 + KCHUNK, j0, tid);   // in flight while this chunk is contracted
#pragma unroll
    for (int kk = 0; kk < KCHUNK; ++kk) {
      double a[MR], s[4];
#pragma unroll
      for (int r = 0; r < MR; ++r) a[r] = Ks[kk * kpitch + ti + ROW_TILE * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = Ss[kk * PANEL + tj * 4 + c];
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], s[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < MR; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) Wt[(tj * 4 + c) * kpitch + ti + ROW_TILE * r] = acc[r][c];
  __syncthreads();
}

}  // namespace

}  // namespace oe
}  // namespace mwrt
