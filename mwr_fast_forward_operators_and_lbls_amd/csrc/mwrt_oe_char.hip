// mwrt_oe_char.hip -- what an optimal-estimation step says about itself (include/mwrt.h mwrt_oe_gain_device and
// mwrt_oe_product_device; Rodgers 2000, ch. 3).  With W = K Sa and G = K Sa K^T + Se = L L^T on the rows kept,
//     gain^T = G^-1 W   [m][n]     A = gain K   [n][n]     S^ = Sa - gain W   [n][n]
//   k_char_gain<MR>   steps 1-4 of k_oe_step (state check, row rule, G in panels, + Se, Cholesky), L^-1 in place, then per
//                     32-column panel W_p again, Z_p = L^-1 W_p and gain^T_p = L^-T Z_p in the same register tiling, and
//                     from the panel in LDS: the rows of gain^T and W, diag A, the noise and the smoothing variance; the
//                     degrees of freedom per state block at the end.  One workgroup of 256 threads per profile.
//   k_char_product    C[p] = L[p]^T R[p] contracted over the rows kept, one 64 x 64 tile of the result per workgroup, a
//                     4 x 4 register tile per thread; epilogue C or Sa - C.  One kernel for A (R = K, addressed by block)
//                     and S^ (R = W, one block of n columns).
// Every sum has a fixed order and nothing is shared between workgroups, so a profile's outputs depend on neither its
// batch-mates nor nprof, and an element of a product on neither the tile nor the row window it is computed in.  Plain fp64
// FMAs.  Every step the gain kernel has in common with k_oe_step is that kernel's block (mwrt_oe_blocks.hip.h; DESIGN 4.6
// lists them).
#include "mwrt_oe_char.hip.h"
#include "mwrt_oe_blocks.hip.h"

#include <math.h>

namespace mwrt {
namespace oec {

namespace {

using namespace oe;                        // the blocks; THREADS is the same constant in both namespaces

// every output of a profile that ends early: `v` everywhere (NaN or 0), keep 0, smooth_var = diag Sa when `prior`
__device__ __forceinline__ void fill_profile(const GainArgs& C, int64_t prof, double v, bool prior, uint8_t status, int nobs,
                                             int tid) {
  const OeArgs& A = C.o;
  const size_t mn = (size_t)A.m * A.n;
  if (C.gain) for (size_t e = tid; e < mn; e += THREADS) C.gain[(size_t)prof * mn + e] = v;
  if (C.ksa) for (size_t e = tid; e < mn; e += THREADS) C.ksa[(size_t)prof * mn + e] = v;
  if (C.keep) for (int i = tid; i < A.m; i += THREADS) C.keep[(size_t)prof * A.m + i] = 0;
  for (int k = tid; k < A.n; k += THREADS) {
    const size_t o = (size_t)prof * A.n + k;
    if (C.avk_diag) C.avk_diag[o] = v;
    if (C.noise_var) C.noise_var[o] = v;
    if (C.smooth_var) C.smooth_var[o] = prior ? A.sa[(size_t)k * A.n + k] : v;
  }
  if (C.dfs_block && tid < A.nblk) C.dfs_block[(size_t)prof * A.nblk + tid] = v;
  if (tid == 0) {
    A.status[prof] = status;
    if (A.nobs) A.nobs[prof] = nobs;
  }
}

template <int MR>
__device__ __forceinline__ void char_gain(const GainArgs& C) {
  extern __shared__ double smem[];
  const OeArgs& A = C.o;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  const int m = A.m, n = A.n, nlev = A.nlev;
  const GainPlan P = gain_plan(m);
  const int mp = P.mp, kpitch = P.kpitch;
  double* G = smem + P.g;
  double* Wt = smem + P.wt;
  double* Ks = smem + P.ks;
  double* Ss = smem + P.ss;
  double* part = smem + P.part;
  double* sed = smem + P.sed;
  double* red = smem + P.red;
  int* keep = reinterpret_cast<int*>(smem + P.keep);

  // ---- 1: the state ----
  {
    const double* xp = A.x + (size_t)prof * n;
    const double* xap = A.xa + (A.xa_per_profile ? (size_t)prof * n : 0);
    if (state_bad<false>(xp, xap, n, nullptr, tid)) {
      fill_profile(C, prof, quiet_nan(), false, 0, 0, tid);
      return;
    }
  }

  // ---- 2: rows ----
  for (int i = wave; i < mp; i += THREADS / 64) {
    const Row r = row_rule<false>(A, prof, i, nullptr, lane);
    if (lane == 0) {
      keep[i] = r.keep ? 1 : 0;
      sed[i] = r.keep ? r.sii : 0.0;
    }
  }
  __syncthreads();
  const int m_used = rows_kept(keep, m);
  if (m_used == 0) {                       // nothing observed: the prior
    fill_profile(C, prof, 0.0, true, 3, 0, tid);
    return;
  }

  // ---- 3: G = K Sa K^T ----
  form_G<MR>(A, prof, keep, G, Wt, Ks, Ss, kpitch);

  // ---- 4: + Se, dropped rows, Cholesky ----
  add_se_and_identity_rows(A, keep, sed, G, 1.0, tid);
  if (!cholesky_packed(G, m, tid)) {
    fill_profile(C, prof, quiet_nan(), false, 2, m_used, tid);
    return;
  }
  if (tid == 0) {
    A.status[prof] = 1;
    if (A.nobs) A.nobs[prof] = m_used;
  }
  if (C.keep) for (int i = tid; i < m; i += THREADS) C.keep[(size_t)prof * m + i] = (uint8_t)keep[i];

  // ---- 5: X = L^-1 in place ----
  invert_lower(G, m, tid);

  // ---- 6: per panel W_p, Z_p = X W_p, gain^T_p = X^T Z_p, and what is read off the panel ----
  const size_t mn = (size_t)m * n;
  double* gain_p = C.gain ? C.gain + (size_t)prof * mn : nullptr;
  double* ksa_p = C.ksa ? C.ksa + (size_t)prof * mn : nullptr;
  const bool want_noise = C.noise_var || C.smooth_var;
  const int ti = tid >> 3, tj = tid & 7;
  const int cj = tid & (PANEL - 1), cq = tid >> 5;           // the column sums: PARTS threads per column
  double* colsum = Ks;                                       // [ROW_TILE][PANEL]: Ks and Ss are contiguous, >= 1040 doubles
  if (tid < 4 * PANEL) red[tid] = 0.0;                       // diag A summed per block: red[b][j] for column j of every panel
  for (int j0 = 0; j0 < n; j0 += PANEL) {
    form_panel<MR>(A, prof, keep, j0, Wt, Ks, Ss, kpitch, tid);
    if (ksa_p && j0 + cj < n) {                              // rows of W, contiguous in n: 32 lanes, 32 columns of a row
      double* o = ksa_p + j0 + cj;
      const double* w = Wt + cj * kpitch;
#pragma unroll 1
      for (int i = cq; i < m; i += PARTS) o[(size_t)i * n] = w[i];
    }
    // The two tile products stay written out, here and in k_oe_step's step 7: as one shared function the compiler hoists
    // their addresses differently and k_char_gain<3> goes from 128 to 162 VGPRs, over the budget its test pins.
    double z[MR][4];
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) z[r][c] = 0.0;
    for (int k = 0; k < m; ++k) {                            // Z = X W_p, X lower triangular
      double xr[MR], w[4];
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const int i = ti + ROW_TILE * r;
        xr[r] = (i < m && k <= i) ? G[tri(i, k)] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = Wt[(tj * 4 + c) * kpitch + k];
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[r][c] = fma(xr[r], w[c], z[r][c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < MR; ++r) s = fma(z[r][c], z[r][c], s);
      colsum[ti * PANEL + tj * 4 + c] = s;
    }
    __syncthreads();                                         // W_p has been read by everyone: Z_p takes its place
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) Wt[(tj * 4 + c) * kpitch + ti + ROW_TILE * r] = z[r][c];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) z[r][c] = 0.0;
    for (int k = 0; k < m; ++k) {                            // gain^T = X^T Z_p: X read transposed
      double xr[MR], w[4];
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const int i = ti + ROW_TILE * r;
        xr[r] = (k < m && i <= k) ? G[tri(k, i)] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = Wt[(tj * 4 + c) * kpitch + k];
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[r][c] = fma(xr[r], w[c], z[r][c]);
    }
    __syncthreads();                                         // Z_p has been read by everyone: gain^T_p takes its place
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const int i = ti + ROW_TILE * r;
      const bool live = i < m && keep[i] != 0;               // a dropped row's contribution function is 0
#pragma unroll
      for (int c = 0; c < 4; ++c) Wt[(tj * 4 + c) * kpitch + i] = live ? z[r][c] : 0.0;
    }
    __syncthreads();
    if (gain_p && j0 + cj < n) {                             // rows of gain^T, contiguous in n
      double* o = gain_p + j0 + cj;
      const double* g = Wt + cj * kpitch;
#pragma unroll 1
      for (int i = cq; i < m; i += PARTS) o[(size_t)i * n] = g[i];
    }
    {                                                        // diag A and the noise variance of column j0 + cj, rows cq + 8 q
      double a = 0.0, s = 0.0;
      const int j = j0 + cj;
      if (j < n) {
        const int b = j / nlev;
        const double* col = kblock(A, b, prof) + (j - b * nlev);
        const double* g = Wt + cj * kpitch;
#pragma unroll 1
        for (int i = cq; i < m; i += PARTS) {
          if (!keep[i]) continue;                            // a dropped row of K is never read: it may hold NaN
          const double gv = g[i];
          a = fma(gv, col[(size_t)i * nlev], a);
          if (want_noise) {
            if (A.se_full) {
              double t = 0.0;
#pragma unroll 2
              for (int c = 0; c < m; ++c)
                if (keep[c]) t = fma(A.se[(size_t)i * m + c], g[c], t);
              s = fma(gv, t, s);
            } else {
              s = fma(sed[i] * gv, gv, s);
            }
          }
        }
      }
      part[cq * PANEL + cj] = a;
      part[(PARTS + cq) * PANEL + cj] = s;
    }
    __syncthreads();
    if (tid < PANEL && j0 + tid < n) {
      const int j = j0 + tid;
      double a = 0.0, s = 0.0;
#pragma unroll 4
      for (int q = 0; q < PARTS; ++q) { a += part[q * PANEL + tid]; s += part[(PARTS + q) * PANEL + tid]; }
      const double zz = column_total(colsum, tid);
      const size_t o = (size_t)prof * n + j;
      if (C.avk_diag) C.avk_diag[o] = a;
      if (C.noise_var) C.noise_var[o] = s;
      if (C.smooth_var) C.smooth_var[o] = A.sa[(size_t)j * n + j] - zz - s;
      red[(j / nlev) * PANEL + tid] += a;
    }
    __syncthreads();                                         // the next panel overwrites Wt, the column sums and part
  }

  // ---- 7: degrees of freedom per block, in the fixed tree ----
  if (C.dfs_block) {
    const double mine = tid < 4 * PANEL ? red[tid] : 0.0;    // thread b * 32 + j holds block b's share of columns j + 32 p
    __syncthreads();
    for (int b = 0; b < A.nblk; ++b) {
      const double v = block_sum(tid >> 5 == b ? mine : 0.0, red, tid);
      if (tid == 0) C.dfs_block[(size_t)prof * A.nblk + b] = v;
    }
  }
}

// The instantiations are held to the register budget of k_oe_step<MR> (what tests/test_oe_kernel_resources.py pins): left
// alone, the compiler spends registers up to the next occupancy step on hoisted addresses of the panel stores.
template <int MR> __global__ void k_char_gain(const GainArgs C);
#define MWRT_CHAR_GAIN(MR, VGPRS) \
  template <> __global__ void __launch_bounds__(THREADS) __attribute__((amdgpu_num_vgpr(VGPRS))) k_char_gain<MR>(const GainArgs C) { char_gain<MR>(C); }
MWRT_CHAR_GAIN(1, 113)
MWRT_CHAR_GAIN(2, 117)
MWRT_CHAR_GAIN(3, 129)
MWRT_CHAR_GAIN(4, 169)
MWRT_CHAR_GAIN(5, 171)
#undef MWRT_CHAR_GAIN

// right operand block b of this profile: entry [i][c] is at base[i * rcols + c]
__device__ __forceinline__ const double* rblock(const ProductArgs& P, int b, int64_t prof) {
  const double* p = b == 0 ? P.r0 : b == 1 ? P.r1 : b == 2 ? P.r2 : P.r3;
  return p + (size_t)prof * P.m * P.rcols;
}

__global__ void __launch_bounds__(THREADS)
k_char_product(const ProductArgs P) {
  extern __shared__ double smem[];
  double* Ls = smem;                                         // [PCHUNK][TILE] rows of the left operand, columns of the tile's rows
  double* Rs = smem + PCHUNK * TILE;                         // [PCHUNK][TILE] rows of the right operand
  const int tid = threadIdx.x;
  const int m = P.m, n = P.n;
  const int64_t tiles = (int64_t)P.tiles_x * P.tiles_y;
  const int64_t prof = (int64_t)blockIdx.x / tiles;
  const int t = (int)((int64_t)blockIdx.x - prof * tiles);
  const int tyl = t / P.tiles_x;
  const int j0 = P.row_begin + tyl * TILE, k0 = (t - tyl * P.tiles_x) * TILE;
  const int jend = P.row_begin + P.rows;

  // a thread loads column lc of both operands' chunks, rows lr + 4 q: consecutive lanes, consecutive addresses
  const int lc = tid & (TILE - 1), lr = tid >> 6;
  const bool lok = j0 + lc < jend, rok = k0 + lc < n;
  const double* lp = P.left + (size_t)prof * m * n + (lok ? j0 + lc : 0);
  const int rb = rok ? (k0 + lc) / P.rcols : 0;
  const double* rp = rblock(P, rb, prof) + (rok ? k0 + lc - rb * P.rcols : 0);
  const uint8_t* keep = P.keep + (size_t)prof * m;
  double lv[4], rv[4];
  auto fetch = [&](int i0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + lr + 4 * q;
      const bool live = i < m && keep[i] != 0;               // a dropped row of either operand is never read
      lv[q] = live && lok ? lp[(size_t)i * n] : 0.0;
      rv[q] = live && rok ? rp[(size_t)i * P.rcols] : 0.0;
    }
  };

  const int cy = tid >> 4, cx = tid & 15;                    // the thread's rows cy + 16 a and columns cx + 16 c of the tile
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
  fetch(0);
  for (int i0 = 0; i0 < m; i0 += PCHUNK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Ls[(lr + 4 * q) * TILE + lc] = lv[q];
      Rs[(lr + 4 * q) * TILE + lc] = rv[q];
    }
    __syncthreads();
    if (i0 + PCHUNK < m) fetch(i0 + PCHUNK);                 // in flight while this chunk is contracted
#pragma unroll
    for (int ii = 0; ii < PCHUNK; ++ii) {
      double a4[4], b4[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) a4[a] = Ls[ii * TILE + cy + 16 * a];
#pragma unroll
      for (int c = 0; c < 4; ++c) b4[c] = Rs[ii * TILE + cx + 16 * c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = fma(a4[a], b4[c], acc[a][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int j = j0 + cy + 16 * a;
    if (j >= jend) continue;
    double* orow = P.out + ((size_t)prof * P.rows + (j - P.row_begin)) * n;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k0 + cx + 16 * c;
      if (k < n) orow[k] = P.sa ? P.sa[(size_t)j * n + k] - acc[a][c] : acc[a][c];
    }
  }
}

}  // namespace

hipError_t launch_char_gain(const GainArgs& a, int64_t nprof, hipStream_t st) {
  const size_t lds = gain_plan(a.o.m).total_bytes;
  switch ((a.o.m + ROW_TILE - 1) / ROW_TILE) {
    case 1: return launch_raised<k_char_gain<1>>(a, nprof, lds, st);
    case 2: return launch_raised<k_char_gain<2>>(a, nprof, lds, st);
    case 3: return launch_raised<k_char_gain<3>>(a, nprof, lds, st);
    case 4: return launch_raised<k_char_gain<4>>(a, nprof, lds, st);
    case 5: return launch_raised<k_char_gain<5>>(a, nprof, lds, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_char_product(const ProductArgs& a, int64_t nprof, hipStream_t st) {
  const int64_t blocks = (int64_t)a.tiles_x * a.tiles_y * nprof;
  if (a.m > MWRT_OE_MAX_M || blocks < 1 || blocks > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_char_product, dim3((unsigned)blocks), dim3(THREADS), PRODUCT_LDS_BYTES, st, a);
  return hipGetLastError();
}

}  // namespace oec
}  // namespace mwrt
