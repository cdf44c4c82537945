// mwrt_nform_char.hip -- the characterisation of the n-form step (include/mwrt.h mwrt_oe_nform_char_device and
// mwrt_oe_nform_gain_device).  At gamma = 0, with H = K^T W K of a linearisation and C = H + Sa^-1 = L L^T:
//     S^ = C^-1,   A = S^ H,   gain^T = W K S^ (row i = S^ k_i / se_i),   noise = diag(A S^),   smooth = diag S^ - noise
//   k_nfc_char   one workgroup per profile: C packed in LDS, Cholesky, L^-1, S^ packed in LDS beside it; H then takes the
//                place of L^-1 and A = S^ H is formed row by row, a wave per row and a lane per column (and column + 64),
//                with both operands in LDS.  Only the rows a call needs are formed: the window of d_avk, and all of them
//                when the noise / smoothing split is asked for; the diagonal of A alone costs n^2.
//   k_nfc_gain   the hot path: per profile the [m][n] x [n][n] product K S^ with the row rule and 1 / se_i applied as the
//                rows are fetched.  The tile plan of k_project (csrc/mwrt_basis.hip): 128 x 32 tiles, the contraction
//                staged through LDS in chunks of 16 with the next chunk's loads in flight, 4 x 4 register tiles; a row
//                tile never leaves its profile (grid: profile x row tile, column tile) and the right matrix is that
//                profile's S^.
// No atomics, no MFMA, no workspace, no scratch.  Every sum has the fixed order mwrt_nform_char.hip.h states, so an element
// is the same bit for bit whatever nprof, the row window, the tile it falls in or the outputs asked for.  The
// factorisation, the inverse of the factor and the block sum are the blocks of mwrt_oe_blocks.hip.h, unchanged.  Every
// global index is 64-bit.
#include "mwrt_nform_char.hip.h"
#include "mwrt_oe_blocks.hip.h"

#include <math.h>

namespace mwrt {
namespace nfc {

namespace {

using namespace oe;                        // the blocks; THREADS is the same constant in both namespaces

// the row of packed entry e: e = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ int tri_row(int e) {
  int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > e) --i;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  return i;
}
// entry (i, j) of a symmetric matrix held as its packed lower triangle
__device__ __forceinline__ int sym(int i, int j) { return i >= j ? tri(i, j) : tri(j, i); }

// `v` into every floating-point output of the profile that was asked for; S^ too unless `keep_cov`
__device__ __forceinline__ void fill_outputs(const CharArgs& A, int64_t prof, double v, bool keep_cov, int tid) {
  const int n = A.n;
  if (A.post_cov && !keep_cov)
    for (int e = tid; e < n * n; e += THREADS) A.post_cov[(size_t)prof * n * n + e] = v;
  if (A.avk)
    for (int e = tid; e < A.rows * n; e += THREADS) A.avk[(size_t)prof * A.rows * n + e] = v;
  for (int k = tid; k < n; k += THREADS) {
    if (A.avk_diag) A.avk_diag[(size_t)prof * n + k] = v;
    if (A.noise_var) A.noise_var[(size_t)prof * n + k] = v;
    if (A.smooth_var && !keep_cov) A.smooth_var[(size_t)prof * n + k] = v;
  }
  if (A.dfs_block && tid < A.nblk) A.dfs_block[(size_t)prof * A.nblk + tid] = v;
}

// ---- S^, A, the budget and the degrees of freedom per block of one linearisation ----
__global__ void __launch_bounds__(THREADS)
k_nfc_char(const CharArgs A) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t prof = blockIdx.x;
  if (A.active && A.active[prof] == 0) return;
  const int n = A.n;
  const CharPlan P = char_plan(n);
  double* C = smem + P.c;                  // C, L, L^-1, then H
  double* S = smem + P.s;                  // S^ packed
  double* dg = smem + P.dg;                // diag A
  double* red = smem + P.red;

  const int nt = n * (n + 1) / 2;
  const double* hin = A.h + (size_t)prof * nt;
  const int lin = A.lin_status[prof];
  if (lin != 1 && lin != 3) {              // 0: the state was not finite; anything else fails as 2
    fill_outputs(A, prof, quiet_nan(), false, tid);
    if (tid == 0) A.status[prof] = lin == 0 ? 0 : 2;
    return;
  }
  const bool nothing = lin == 3;           // no usable row: H = 0, whatever the buffer holds

  // ---- C = H + Sa^-1 (the sum the solve forms at gamma = 0); Cholesky; L^-1 ----
  for (int i = tid >> 4; i < n; i += THREADS / 16)
    for (int c = tid & 15; c <= i; c += 16)
      C[tri(i, c)] = fma(1.0, A.sa_inv[(size_t)i * n + c], nothing ? 0.0 : hin[tri(i, c)]);
  __syncthreads();
  if (!cholesky_packed(C, n, tid)) {
    fill_outputs(A, prof, quiet_nan(), false, tid);
    if (nothing) fill_outputs(A, prof, 0.0, true, tid);      // A and what is summed from it stay 0; S^ and smooth NaN
    if (tid == 0) A.status[prof] = nothing ? 3 : 2;
    return;
  }
  invert_lower(C, n, tid);

  // ---- S^ = L^-T L^-1 element by element, as k_nf_solve forms it ----
  for (int e = tid; e < nt; e += THREADS) {
    const int i = tri_row(e), j = e - i * (i + 1) / 2;
    double cinv = 0.0;
    for (int k = i; k < n; ++k) cinv = fma(C[tri(k, i)], C[tri(k, j)], cinv);
    S[e] = cinv;
    if (A.post_cov) {
      A.post_cov[(size_t)prof * n * n + (size_t)i * n + j] = cinv;
      A.post_cov[(size_t)prof * n * n + (size_t)j * n + i] = cinv;
    }
  }
  __syncthreads();
  if (nothing) {                           // A = 0 exactly; the posterior is the prior as computed
    fill_outputs(A, prof, 0.0, true, tid);
    if (A.smooth_var)
      for (int k = tid; k < n; k += THREADS) A.smooth_var[(size_t)prof * n + k] = S[tri(k, k)];
    if (tid == 0) A.status[prof] = 3;
    return;
  }

  // ---- H packed in the place of L^-1 ----
  for (int e = tid; e < nt; e += THREADS) C[e] = hin[e];
  __syncthreads();
  const double* H = C;

  // ---- diag A, one thread per entry: the chain of A[j][j] below ----
  if (A.avk_diag || A.dfs_block) {
    for (int j = tid; j < n; j += THREADS) {
      double a = 0.0;
      for (int l = 0; l < n; ++l) a = fma(S[sym(j, l)], H[sym(l, j)], a);
      dg[j] = a;
      if (A.avk_diag) A.avk_diag[(size_t)prof * n + j] = a;
    }
    __syncthreads();
    if (A.dfs_block) {
      for (int b = 0; b < A.nblk; ++b) {
        const bool in = tid >= b * A.nlev && tid < (b + 1) * A.nlev;
        const double d = block_sum(in ? dg[tid] : 0.0, red, tid);
        if (tid == 0) A.dfs_block[(size_t)prof * A.nblk + b] = d;
      }
    }
  }

  // ---- the rows of A a call needs: wave w forms rows w, w + 4, ...; lane l the columns l and l + 64 ----
  const bool budget = A.noise_var || A.smooth_var;
  if (A.avk || budget) {
    const bool two = n > 64;                                   // uniform: the second column of a lane exists
    const bool in0 = lane < n, in1 = lane + 64 < n;
    const int k0 = in0 ? lane : 0, k1 = in1 ? lane + 64 : 0;  // a lane beyond n reads column 0 and stores nothing
    const int t0 = k0 * (k0 + 1) / 2, t1 = k1 * (k1 + 1) / 2;
    for (int j = wave; j < n; j += THREADS / 64) {
      const bool window = A.avk && j >= A.row_begin && j < A.row_begin + A.rows;
      if (!window && !budget) continue;                        // uniform over the wave
      double a0 = 0.0, a1 = 0.0;
      const int tj = j * (j + 1) / 2;
      for (int l = 0; l < n; ++l) {
        const int tl = l * (l + 1) / 2;
        const double s = S[j >= l ? tj + l : tl + j];
        a0 = fma(s, H[l >= k0 ? tl + k0 : t0 + l], a0);
        if (two) a1 = fma(s, H[l >= k1 ? tl + k1 : t1 + l], a1);
      }
      if (window) {
        double* row = A.avk + ((size_t)prof * A.rows + (j - A.row_begin)) * n;
        if (in0) row[lane] = a0;
        if (in1) row[lane + 64] = a1;
      }
      if (budget) {
        double part = in0 ? a0 * S[sym(k0, j)] : 0.0;
        if (in1) part = fma(a1, S[sym(k1, j)], part);
        const double noise = wave_sum(part);
        if (lane == 0) {
          if (A.noise_var) A.noise_var[(size_t)prof * n + j] = noise;
          if (A.smooth_var) A.smooth_var[(size_t)prof * n + j] = S[tj + j] - noise;
        }
      }
    }
  }
  if (tid == 0) A.status[prof] = 1;
}

// one contraction chunk on its way from global memory to LDS: 2 MR elements of the rows and two of S^ per thread
struct Chunk {
  double k[2 * MR], s[2];
  __device__ __forceinline__ void fetch(const CharArgs& A, const double* sp, int64_t rbase, int row0, const bool (&kept)[2 * MR],
                                        const double (&w)[2 * MR], int k0, int j0, int tid) {
    const int lkk = tid & (KCHUNK - 1), li = tid / KCHUNK;
    const int kk = k0 + lkk;
    const bool kin = kk < A.n;
    const int b = kin ? kk / A.nlev : 0;
    const int l = kin ? kk - b * A.nlev : 0;
    const double* base = (b == 0 ? A.k0 : b == 1 ? A.k1 : b == 2 ? A.k2 : A.k3) + l;
#pragma unroll
    for (int q = 0; q < 2 * MR; ++q) {
      const int row = row0 + li + (THREADS / KCHUNK) * q;
      const double v = (kin && row < A.m) ? base[(rbase + row) * A.nlev] : 0.0;
      k[q] = kept[q] ? v * w[q] : 0.0;                         // the select after the load: a dropped row may hold NaN
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + THREADS * q;
      const int kr = k0 + e / COLS, jc = j0 + (e & (COLS - 1));
      s[q] = (kr < A.n && jc < A.n) ? sp[(size_t)kr * A.n + jc] : 0.0;
    }
  }
  __device__ __forceinline__ void store(double* Ks, double* Ss, int tid) const {
    const int lkk = tid & (KCHUNK - 1), li = tid / KCHUNK;
#pragma unroll
    for (int q = 0; q < 2 * MR; ++q) Ks[lkk * KPITCH + li + (THREADS / KCHUNK) * q] = k[q];
#pragma unroll
    for (int q = 0; q < 2; ++q) Ss[tid + THREADS * q] = s[q];
  }
};

// ---- gain^T = W K S^ ----
__global__ void __launch_bounds__(THREADS)
k_nfc_gain(const CharArgs A, const int row_tiles) {
  __shared__ double Ks[KCHUNK * KPITCH];
  __shared__ double Ss[KCHUNK * COLS];
  const int tid = threadIdx.x;
  const int ti = tid >> 3, tj = tid & 7;
  const int64_t prof = blockIdx.x / (unsigned)row_tiles;
  if (A.active && A.active[prof] == 0) return;
  const int row0 = (int)(blockIdx.x - (unsigned)(prof * row_tiles)) * ROWS;   // < m + ROWS: row_tiles * ROWS < 2^31 + ROWS
  const int j0 = (int)blockIdx.y * COLS;
  const int m = A.m, n = A.n;
  const int64_t rbase = prof * m;
  double* out = A.gain + rbase * n;

  const int status = A.status[prof];
  if (status != 1) {                       // 3: no row was used, 0 exactly; else the profile failed: NaN
    const double v = status == 3 ? 0.0 : quiet_nan();
    for (int e = tid; e < ROWS * COLS; e += THREADS) {
      const int64_t row = (int64_t)row0 + e / COLS;
      const int j = j0 + (e & (COLS - 1));
      if (row < m && j < n) out[row * n + j] = v;
    }
    return;
  }

  // the thread's rows of a chunk: the row rule as prepare decided it and 1 / se_i
  const uint8_t* keep = A.keep + rbase;
  const double* sep = A.se + (A.se_per_profile ? rbase : 0);
  bool kept[2 * MR];
  double w[2 * MR];
#pragma unroll
  for (int q = 0; q < 2 * MR; ++q) {
    const int64_t row = (int64_t)row0 + tid / KCHUNK + (THREADS / KCHUNK) * q;
    kept[q] = row < m && keep[row] != 0;
    w[q] = kept[q] ? 1.0 / sep[row] : 0.0;
  }
  const double* sp = A.post_cov + (size_t)prof * n * n;

  double acc[MR][NC];
#pragma unroll
  for (int q = 0; q < MR; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[q][c] = 0.0;
  Chunk ch;
  ch.fetch(A, sp, rbase, row0, kept, w, 0, j0, tid);
  for (int k0 = 0; k0 < n; k0 += KCHUNK) {
    ch.store(Ks, Ss, tid);
    __syncthreads();
    if (k0 + KCHUNK < n) ch.fetch(A, sp, rbase, row0, kept, w, k0 + KCHUNK, j0, tid);   // in flight while this chunk is contracted
#pragma unroll
    for (int kk = 0; kk < KCHUNK; ++kk) {
      double a[MR], s[NC];
#pragma unroll
      for (int q = 0; q < MR; ++q) a[q] = Ks[kk * KPITCH + ti + (THREADS / 8) * q];
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = Ss[kk * COLS + tj * NC + c];
#pragma unroll
      for (int q = 0; q < MR; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[q][c] = fma(a[q], s[c], acc[q][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < MR; ++q) {
    const int64_t row = (int64_t)row0 + ti + (THREADS / 8) * q;
    if (row >= m) continue;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = j0 + tj * NC + c;
      if (j < n) out[row * n + j] = acc[q][c];
    }
  }
}

}  // namespace

hipError_t launch_nfc_char(const CharArgs& a, int64_t nprof, hipStream_t st) {
  if (a.n > MWRT_OE_NFORM_MAX_N) return hipErrorInvalidValue;
  return launch_raised<k_nfc_char>(a, nprof, char_plan(a.n).total_bytes, st);
}

hipError_t launch_nfc_gain(const CharArgs& a, int64_t nprof, hipStream_t st) {
  if (a.n > MWRT_OE_NFORM_MAX_N) return hipErrorInvalidValue;
  const int64_t rt = gain_row_tiles(a.m);
  if (nprof < 1 || nprof > 2147483647LL / rt) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_nfc_gain, dim3((unsigned)(nprof * rt), (unsigned)gain_col_tiles(a.n)), dim3(THREADS), 0, st, a, (int)rt);
  return hipGetLastError();
}

}  // namespace nfc
}  // namespace mwrt
