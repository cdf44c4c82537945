// mwrt_whiten.hip -- pre-whitening with a per-profile observation-error covariance (include/mwrt.h
// mwrt_obs_whiten_device / mwrt_obs_whiten_apply_device).  With Se_p = L_p L_p^T on the rows profile p keeps,
//     K~ = L^-1 K,   y~ = L^-1 y,   F~ = L^-1 F(x)
// make the optimal-estimation entries, called with Se = 1, compute the step of Se_p; gain = L^-T gain~ restores the gain.
//   k_wh_factor  one workgroup per profile: the row rule of mwrt_oe_step_device (one wave per row), the kept Se_p as a
//                packed lower triangle in LDS with a dropped row a row of the identity, cholesky_packed, then L, keep and
//                status to global memory.
//   k_wh_apply   one wave per (profile, tile of COLS columns), lanes along the level axis.  The tile is loaded into LDS
//                once (vt [m][COLS], LOAD_BATCH rows in flight together) and solved there in place, ROW_BLOCK rows abreast:
//                L^-1 gathers the solved rows into ROW_BLOCK FMA chains (one LDS read feeds all of them), L^-T scatters
//                ROW_BLOCK solved rows onto the rows before them -- either way L is walked along its rows, which are
//                contiguous: the rows of a block are staged in LDS one block ahead and L_ij, uniform over the wave, is
//                an LDS broadcast.  A lane touches its own column alone, so the kernel has no barrier.  The two
//                vectors are lanes 0 and 1 of one more tile.
// No atomics, no workspace, no scratch, plain fp64 FMAs.  Every output element is one FMA chain in the order
// mwrt_whiten.hip.h states, fed by its own column and its profile's L alone: the same bit for bit whatever nprof, the tile
// it falls in, the outputs asked for, or the call.  Every global index is 64-bit.
#include "mwrt_whiten.hip.h"
#include "mwrt_oe_blocks.hip.h"

namespace mwrt {
namespace wh {

static_assert(FACTOR_THREADS == oe::THREADS, "cholesky_packed strides by oe::THREADS");
static_assert(MWRT_OE_MAX_M <= 64 * KEEP_WORDS, "the row flags fit the masks");

namespace {

using oe::finite_f64;
using oe::quiet_nan;
using oe::tri;

__global__ void __launch_bounds__(FACTOR_THREADS)
k_wh_factor(const FactorArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = A.m, nlev = A.nlev;
  const int64_t p = blockIdx.x;
  const int ng = m * (m + 1) / 2;
  double* G = lds;
  int* keep = reinterpret_cast<int*>(lds + ((ng + 1) & ~1));
  // the row rule, one wave per row
  for (int i = wave; i < m; i += FACTOR_THREADS / 64) {
    const int64_t row = p * m + i;
    bool ok = finite_f64(A.y[row]) && finite_f64(A.fx[row]);
    if (A.se_full) {
      for (int c = lane; c < m; c += 64) ok = ok && finite_f64(A.se[row * m + c]);
    } else {
      ok = ok && finite_f64(A.se[row]);
    }
    for (int b = 0; b < A.nblk; ++b) {
      const double* kr = (b == 0 ? A.k0 : b == 1 ? A.k1 : b == 2 ? A.k2 : A.k3) + row * nlev;
      for (int l = lane; l < nlev; l += 64) ok = ok && finite_f64(kr[l]);
    }
    const bool k = __all(ok);
    if (lane == 0) keep[i] = k;
  }
  __syncthreads();
  const int m_used = oe::rows_kept(keep, m);
  // Se_p on the rows and columns kept, loaded first and selected afterwards; a dropped row is a row of the identity
  for (int i = tid >> 4; i < m; i += FACTOR_THREADS / 16)
    for (int c = tid & 15; c <= i; c += 16) {
      const double v = A.se_full ? A.se[(p * m + i) * m + c] : (c == i ? A.se[p * m + i] : 0.0);
      G[tri(i, c)] = (keep[i] && keep[c]) ? v : (c == i ? 1.0 : 0.0);
    }
  __syncthreads();
  const bool ok = m_used == 0 || oe::cholesky_packed(G, m, tid);   // nothing kept: G is the identity, and so is L
  double* lp = A.l + p * ng;
  for (int e = tid; e < ng; e += FACTOR_THREADS) lp[e] = ok ? G[e] : quiet_nan();
  for (int i = tid; i < m; i += FACTOR_THREADS) A.keep[p * m + i] = (uint8_t)(ok ? keep[i] : 0);
  if (tid == 0) A.status[p] = (uint8_t)(!ok ? 2 : m_used == 0 ? 3 : 1);
}

// row i's flag out of the masks
__device__ __forceinline__ bool kept(unsigned long long kw0, unsigned long long kw1, unsigned long long kw2, int i) {
  return ((i < 64 ? kw0 : i < 128 ? kw1 : kw2) >> (i & 63)) & 1;
}

// mode 0, rows i0 .. i0 + RB - 1 of the tile; the rows before i0 are solved
template <int RB>
__device__ __forceinline__ void forward_rows(double* vt, const double* lp, int i0, double (&t)[RB]) {
  double acc[RB];
  const double* lr[RB];
#pragma unroll
  for (int q = 0; q < RB; ++q) {
    acc[q] = vt[(i0 + q) * COLS];
    lr[q] = lp + tri(i0 + q, 0);
  }
  for (int j = 0; j < i0; ++j) {
    const double w = vt[j * COLS];
#pragma unroll
    for (int q = 0; q < RB; ++q) acc[q] = fma(-lr[q][j], w, acc[q]);
  }
#pragma unroll
  for (int q = 0; q < RB; ++q) {
#pragma unroll
    for (int s = 0; s < q; ++s) acc[q] = fma(-lr[q][i0 + s], t[s], acc[q]);
    t[q] = acc[q] / lr[q][i0 + q];
  }
}

// mode 1, rows j0 .. j0 + RB - 1, to which every row behind them has been applied already: solve them (descending), then
// take them off every row before j0 -- row j of L is contiguous, a column is not, so here the solved rows go to the
// unsolved ones.  Row i < j0 still meets its rows j > i in descending order, one FMA each.  `live`: the block's row flags.
template <int RB>
__device__ __forceinline__ void transposed_rows(double* vt, const double* lp, int j0, const bool (&live)[RB], double (&t)[RB]) {
  double acc[RB];
  const double* lr[RB];
#pragma unroll
  for (int q = 0; q < RB; ++q) {
    acc[q] = vt[(j0 + q) * COLS];
    lr[q] = lp + tri(j0 + q, 0);
  }
#pragma unroll
  for (int q = RB - 1; q >= 0; --q) {
#pragma unroll
    for (int s = RB - 1; s > q; --s) acc[q] = fma(-lr[s][j0 + q], t[s], acc[q]);
    acc[q] = acc[q] / lr[q][j0 + q];
    t[q] = live[q] ? acc[q] : 0.0;                          // a dropped row takes part as 0
  }
  for (int i = 0; i < j0; ++i) {
    double v = vt[i * COLS];
#pragma unroll
    for (int s = RB - 1; s >= 0; --s) v = fma(-lr[s][i], t[s], v);
    vt[i * COLS] = v;
  }
}

__global__ void __launch_bounds__(COLS)
k_wh_apply(const ApplyArgs A, const double* __restrict__ l, const uint8_t* __restrict__ keep) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, m = A.m;
  const int64_t p = blockIdx.x / (unsigned)A.tiles;
  const int tile = (int)(blockIdx.x - p * A.tiles);
  // this lane's column: where it comes from, where it goes and the distance between its rows
  const double* src = nullptr;
  double* dst = nullptr;
  int pitch = 1;
  const bool vec = tile >= A.nblk * A.ctiles;
  if (vec) {
    if (lane < 2) {
      src = lane == 0 ? A.v_in0 : A.v_in1;
      dst = lane == 0 ? A.v_out0 : A.v_out1;
      if (src) src += p * m;
      if (dst) dst += p * m;
    }
  } else {
    const int b = tile / A.ctiles, col = (tile - b * A.ctiles) * COLS + lane;
    if (col < A.nlev) {
      pitch = A.nlev;
      src = (b == 0 ? A.in0 : b == 1 ? A.in1 : b == 2 ? A.in2 : A.in3) + p * m * A.nlev + col;
      dst = (b == 0 ? A.out0 : b == 1 ? A.out1 : b == 2 ? A.out2 : A.out3) + p * m * A.nlev + col;
    }
  }
  // L and keep are parameters of their own, restrict-qualified: no store of this kernel can reach them
  const double* lp = l + p * (m * (m + 1) / 2);
  const uint8_t* kp = keep + p * m;
  // the row flags as masks, the same in every lane
  const unsigned long long kw0 = __ballot(lane < m && kp[lane] != 0);
  const unsigned long long kw1 = __ballot(64 + lane < m && kp[64 + lane] != 0);
  const unsigned long long kw2 = __ballot(128 + lane < m && kp[128 + lane] != 0);
  const double l00 = lp[0];
  const bool failed = l00 != l00;                          // the factorisation gave status 2: NaN everywhere
  const double dropped = (failed || vec) ? quiet_nan() : 0.0;
  double* vt = lds + lane;                                  // vt[i * COLS]: row i of this lane's column
  // The tile into LDS, LOAD_BATCH rows in flight at a time: loads first, the select after (a dropped row may hold NaN).
  // Every load is unconditional, so that none waits for another: a lane without a column reads L[0] again and again, and
  // the last batch reads row m - 1 for the rows beyond it.
  const double* from = src ? src : lp;
  const int64_t step = src ? pitch : 0;
  for (int i0 = 0; i0 < m; i0 += LOAD_BATCH) {
    double v[LOAD_BATCH];
#pragma unroll
    for (int q = 0; q < LOAD_BATCH; ++q) v[q] = from[(i0 + q < m ? i0 + q : m - 1) * step];
#pragma unroll
    for (int q = 0; q < LOAD_BATCH; ++q)
      if (i0 + q < m) vt[(i0 + q) * COLS] = kept(kw0, kw1, kw2, i0 + q) ? v[q] : 0.0;
  }
  const int full = m - m % ROW_BLOCK;
  auto put = [=](int i, double w) {
    const bool k = kept(kw0, kw1, kw2, i);
    vt[i * COLS] = k ? w : 0.0;
    if (dst) dst[(int64_t)i * pitch] = k ? w : dropped;
  };
  // The rows of L a block of rows needs -- rows r0 .. r0 + rb - 1 up to their diagonals, contiguous in the packed triangle --
  // are staged in LDS behind the tile (ls), read from there at a uniform address (a broadcast), and fetched one block ahead
  // into registers, so that the latency of L is paid beside the block before and not inside every step of the chains.
  double* ls = lds + (size_t)m * COLS;
  double ahead[STAGE_REGS];
  auto fetch = [&](int r0, int rb) {
    const int base = tri(r0, 0), last = tri(r0 + rb - 1, r0 + rb - 1) - base;
#pragma unroll
    for (int q = 0; q < STAGE_REGS; ++q) ahead[q] = lp[base + min(lane + COLS * q, last)];
  };
  auto stash = [&](int r0, int rb) {
    const int count = tri(r0 + rb - 1, r0 + rb - 1) - tri(r0, 0) + 1;
#pragma unroll
    for (int q = 0; q < STAGE_REGS; ++q)
      if (lane + COLS * q < count) ls[lane + COLS * q] = ahead[q];
  };
  if (A.mode == 0) {
    if (full > 0) fetch(0, ROW_BLOCK);
    for (int i0 = 0; i0 < full; i0 += ROW_BLOCK) {
      stash(i0, ROW_BLOCK);
      if (i0 + ROW_BLOCK < full) fetch(i0 + ROW_BLOCK, ROW_BLOCK);
      double t[ROW_BLOCK];
      forward_rows<ROW_BLOCK>(vt, ls - tri(i0, 0), i0, t);
#pragma unroll
      for (int q = 0; q < ROW_BLOCK; ++q) put(i0 + q, t[q]);
    }
    for (int i = full; i < m; ++i) {
      double t[1];
      fetch(i, 1);
      stash(i, 1);
      forward_rows<1>(vt, ls - tri(i, 0), i, t);
      put(i, t[0]);
    }
  } else {
    if (full > 0) fetch(m - ROW_BLOCK, ROW_BLOCK);
    for (int i0 = m - ROW_BLOCK; i0 >= m - full; i0 -= ROW_BLOCK) {
      stash(i0, ROW_BLOCK);
      if (i0 - ROW_BLOCK >= m - full) fetch(i0 - ROW_BLOCK, ROW_BLOCK);
      double t[ROW_BLOCK];
      bool live[ROW_BLOCK];
#pragma unroll
      for (int q = 0; q < ROW_BLOCK; ++q) live[q] = kept(kw0, kw1, kw2, i0 + q);
      transposed_rows<ROW_BLOCK>(vt, ls - tri(i0, 0), i0, live, t);
#pragma unroll
      for (int q = ROW_BLOCK - 1; q >= 0; --q) put(i0 + q, t[q]);
    }
    for (int i = m - full - 1; i >= 0; --i) {
      double t[1];
      const bool live[1] = {kept(kw0, kw1, kw2, i)};
      fetch(i, 1);
      stash(i, 1);
      transposed_rows<1>(vt, ls - tri(i, 0), i, live, t);
      put(i, t[0]);
    }
  }
}

// Raise `kernel`'s dynamic LDS limit when a launch first needs more than it had on this device, as oe::launch_raised does:
// a repeat call of the same (or a smaller) size is the launch alone.
template <auto kernel>
hipError_t raise_lds(size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  constexpr int MAX_DEV = 64;
  static std::atomic<size_t> raised[MAX_DEV];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= MAX_DEV || raised[dev].load(std::memory_order_acquire) < lds) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < MAX_DEV) raised[dev].store(lds, std::memory_order_release);
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_factor(const FactorArgs& a, int64_t nprof, hipStream_t st) {
  if (nprof < 1 || nprof > 2147483647LL || a.m < 1 || a.m > MWRT_OE_MAX_M) return hipErrorInvalidValue;
  const size_t lds = factor_lds_bytes(a.m);
  if (const hipError_t e = raise_lds<k_wh_factor>(lds)) return e;
  hipLaunchKernelGGL(k_wh_factor, dim3((unsigned)nprof), dim3(FACTOR_THREADS), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_apply(const ApplyArgs& a, int64_t nprof, hipStream_t st) {
  if (nprof < 1 || a.tiles < 1 || nprof > 2147483647LL / a.tiles || a.m < 1 || a.m > MWRT_OE_MAX_M)
    return hipErrorInvalidValue;
  const size_t lds = apply_lds_bytes(a.m);
  if (const hipError_t e = raise_lds<k_wh_apply>(lds)) return e;
  hipLaunchKernelGGL(k_wh_apply, dim3((unsigned)(nprof * a.tiles)), dim3(COLS), lds, st, a, a.l, a.keep);
  return hipGetLastError();
}

}  // namespace wh
}  // namespace mwrt
