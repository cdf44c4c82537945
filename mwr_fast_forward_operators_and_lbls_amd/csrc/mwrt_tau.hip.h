// mwrt_tau.hip.h -- the kernels of the two-step paths: absorption alone or down to zenith layer optical depths
// (k_absorb, k_absorb_win on fine spectral grids) and the RTE that reads those from HBM (k_rte_tau).
#pragma once
#include "mwrt_absorption.hip.h"
#include "mwrt_layer.hip.h"

namespace mwrt {

// ---------------------------------------------------------------------------------------------
// K1 alone: awet / adry [nprof][nf][nlev] (RTEquation.clearsky_absorption [EXT]) -- or, TAU = true, K1 + the layer
// step: zenith layer optical depth tau [nprof][nlev][fpitch] (exponential_integration(zeroflg = True) on wet and
// dry, summed), 8 B per (profile, level, frequency) instead of 16, frequency fastest: what k_rte_tau reads with
// lane = frequency.
//
// TAU-mode level mapping.  The layer step needs level i-1 next to level i.  Lanes are levels, so the neighbour is
// one lane down (a DPP shift, no LDS) -- except across wave seams.  Instead of passing seam values through LDS
// behind a workgroup barrier, each wave REPEATS the last level of the wave below in its lane 0:
//     level(wave, lane) = 63 * wave + lane,    lane 0 of waves >= 1 is a duplicate that stores nothing.
// 3 waves cover 190 levels (the reference's 180), and the waves of a workgroup never wait for each other inside
// the frequency loop.
// ---------------------------------------------------------------------------------------------
// (TAU_NFC and tau_threads, the workgroup size that follows from this mapping: mwrt_plan.h)

// value of lane - 1 (lane 0 keeps its own): GFX9 wave_shr:1, two v_mov_b32_dpp, no LDS crossbar
__device__ __forceinline__ double lane_below(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = (int)b, hi = (int)(b >> 32);
  const int plo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
  const int phi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((long long)phi << 32) | (unsigned)plo);
}

// One chunk of layer optical depths: lane = level holds tz[16] = its row's 16 frequencies = one 128-byte line, written
// in eight 16-byte pieces.  (Transposing 4 x 4 blocks of pieces across each quad of lanes first, so that a store
// instruction has every quad write 64 contiguous bytes, was measured: same-box A/B 3.93 vs 3.82 ms -- the 128 DPP
// moves cost more than the fuller memory requests save; so were nontemporal stores: no difference; a fully coalesced
// (level-fastest, i.e. wrong) layout as a timing experiment: 3.60 / 3.72 vs 3.74 / 3.75 ms -- the pattern is not the cost.)
//   lev0 = level of lane 0 of this wave; a lane's row is stored when `row_ok(level, lane)` (duplicate / padding rows are not).
template <class RowOk>
__device__ __forceinline__ void store_tau_chunk(const double (&tz)[TAU_NFC], double* tau_prof /* + jbase */, int64_t fpitch,
                                                int lev0, int lane, RowOk row_ok) {
  if (row_ok(lev0 + lane, lane)) {
    double2* row = (double2*)(tau_prof + (int64_t)(lev0 + lane) * fpitch);
#pragma unroll
    for (int j = 0; j < TAU_NFC; j += 2) row[j / 2] = double2{tz[j], tz[j + 1]};
  }
}

// the chunk's frequency table {f, f^2} x NFC, {fmin, fmax}, N2 factor x NFC in a WAVE-PRIVATE piece of LDS: filled
// and read by the same wave, so no workgroup barrier separates consecutive chunks
template <int NFC, class ModelPtr>
__device__ __forceinline__ void fill_chunk_table(double* sfq, ModelPtr M, cdoubles cfrq, int jbase, int nfc, int lane) {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");                      // the previous chunk's reads stay above the refill
  if (lane < NFC) {
    const double f = cfrq[jbase + min(lane, nfc - 1)];
    sfq[2 * lane] = f; sfq[2 * lane + 1] = f * f;
    double fdep = 1.0;
    if (M->n2_fdep) { const double q = f * (1.0 / 450.0); fdep = 0.5 + fdiv(0.5, 1.0 + q * q); }
    sfq[2 * NFC + 2 + lane] = fdep;
  }
  if (lane == WAVE - 1) {
    double lo = cfrq[jbase], hi = lo;
    for (int j = 1; j < nfc; ++j) { const double f = cfrq[jbase + j]; lo = fmin(lo, f); hi = fmax(hi, f); }
    sfq[2 * NFC] = lo; sfq[2 * NFC + 1] = hi;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// NaN rows for chunks [c0, c0 + nch) of one profile (NaN input, negative absorption): k_rte_tau turns them into NaN TBs
__device__ __forceinline__ void blank_tau(const TauOut& T, int64_t prof, int nlev, int c0, int nch, int tid, int nthreads) {
  const double qnan = __builtin_nan("");
  const int w = nch * TAU_NFC;
  for (int it = tid; it < nlev * w; it += nthreads) {
    const int l = it / w, k = it - l * w;
    T.tau[(prof * nlev + l) * (int64_t)T.fpitch + c0 * TAU_NFC + k] = qnan;
  }
}

template <int NFC, int MAXT, bool TAU = false>
__global__ void __launch_bounds__(MAXT)
k_absorb(const AbsorbArgs A) {
  static_assert(!TAU || NFC == TAU_NFC, "tau rows are written in 16-frequency pieces");
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int64_t prof = blockIdx.x;
  const int jbase = blockIdx.y * NFC;
  const int nfc = min(NFC, A.nf - jbase);
  const cmodel M = (cmodel)A.M;
  const cdoubles cfrq = (cdoubles)A.frq;
  __shared__ double sfq_w[MAXT / WAVE][3 * NFC + 2];
  double* sfq = sfq_w[wave];
  fill_chunk_table<NFC>(sfq, M, cfrq, jbase, nfc, lane);
  const int lev = TAU ? wave * (WAVE - 1) + lane : tid;
  const bool active = lev < A.nlev;
  const int64_t off = prof * A.nlev + (active ? lev : 0);
  const double pi = A.p[off], ti = A.t[off], rhi = A.rh[off];
  double zi = 0.0;
  if constexpr (TAU) {
    zi = A.T.z[off];
    if (__syncthreads_or(active && (isnan(zi) || isnan(pi) || isnan(ti) || isnan(rhi)))) {   // check_for_nans
      blank_tau(A.T, prof, A.nlev, blockIdx.y, 1, tid, blockDim.x);
      if (tid == 0) A.T.valid[prof] = 0;
      return;
    }
  }
  double awet[NFC], adry[NFC];
  const double e = goff_gratch_e(ti, rhi);
  const LevelState L = level_state(pi, ti, e);
  const LineMasks lm = load_masks(A.masks, blockIdx.y);
  h2o_absorb<NFC>(M, L, sfq, lm, awet);
  dry_absorb<NFC>(M, L, sfq, lm, adry);
  if constexpr (!TAU) {
    if (active) {
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        if (j < nfc) {
          const int64_t o = (prof * A.nf + jbase + j) * A.nlev + tid;
          A.awet[o] = awet[j];
          A.adry[o] = adry[j];
        }
      }
    }
  } else {
    const bool has_prev = active && lev > 0 && lane > 0;
    const double z0 = A.T.z[prof * A.nlev];
    const double dz = has_prev ? ((zi - z0) - (A.T.z[off - 1] - z0)) : 0.0;
    bool neg = false;
    double tz[NFC];
#pragma unroll
    for (int j = 0; j < NFC; j += 4) {
#pragma clang fp contract(off)               // wet * dz + dry * dz rounds as in the fused kernel
      double w4[4] = {awet[j], awet[j + 1], awet[j + 2], awet[j + 3]};
      double d4[4] = {adry[j], adry[j + 1], adry[j + 2], adry[j + 3]};
      const double wb[4] = {lane_below(w4[0]), lane_below(w4[1]), lane_below(w4[2]), lane_below(w4[3])};
      const double db[4] = {lane_below(d4[0]), lane_below(d4[1]), lane_below(d4[2]), lane_below(d4[3])};
      layer_value4(w4, wb, neg, has_prev);
      layer_value4(d4, db, neg, has_prev);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double twj = has_prev ? w4[k] * dz : 0.0;
        const double tdj = has_prev ? d4[k] * dz : 0.0;
        tz[j + k] = twj + tdj;
      }
    }
    {
      const int nlev = A.nlev;
      store_tau_chunk(tz, A.T.tau + prof * nlev * (int64_t)A.T.fpitch + jbase, A.T.fpitch, wave * (WAVE - 1), lane,
                      [&](int l, int ln) { return l < nlev && (ln > 0 || wave == 0); });
    }
    if (__syncthreads_or(neg)) {              // pyrtlib raises ValueError here: flag 2, NaN out
      blank_tau(A.T, prof, A.nlev, blockIdx.y, 1, tid, blockDim.x);
      if (tid == 0) A.T.valid[prof] = 2;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K1 on fine spectral grids: windowed evaluation (k_absorb_win)
//
// On a grid of hundreds of frequencies most of a chunk's 65 lines are far from the whole NEIGHBOURHOOD of the
// chunk, and their sum is an analytic function of f there (poles at c_k +- i w_k, at least WIN_MARGIN_GHZ beyond
// the window's ends).  A workgroup therefore owns a WINDOW of WIN_CHUNKS consecutive 16-frequency chunks of one
// profile: it sums the window-far lines once at WIN_NODES Chebyshev nodes of the window (same line bodies as
// everywhere else), and for each chunk interpolates those sums to the chunk's frequencies with a precomputed
// Lagrange matrix (wave-uniform, from the host: depends on the frequencies only) and adds the remaining lines
// -- near the window, speed dependent, or failing a per-level vote -- directly.  The per-(level, line) setup of
// the far lines is paid once per window instead of once per chunk.
// Interpolation error: what sets it is a strong isolated line just beyond the margin -- 118.7503 GHz seen from
// [122.76, 127.76] or [109.74, 114.74] (4.01 GHz beyond a 5-GHz window, 2.6 half-spans from its middle) leaves
// 2.7e-10 of the dry absorption at the sharp-line top levels, the 6-GHz window [107.95, 113.95] 2.1e-10; inside the
// 60-GHz band, where many far lines share the sum, 3e-11, out of band 1e-13 (tests/window_reference.py
// plan_truncation on the oracle's formulas, held under 5e-10 by tests/test_window_plan.py).  On the device the windowed
// sums then meet the every-line kernel to 3.1e-10 and the oracle to 3.0e-10 relative on those windows (bar 1e-9), TBs to
// 1.4e-9 K (bar 1e-6 K): tests/test_window_geometry.py, profiles/window_geometry_errors.json.
//
// TAU = true: the chunk ends with the layer step (see k_absorb) and writes the zenith layer optical depth,
// [level][frequency], 8 B per point; the fine-grid TB path is this kernel followed by k_rte_tau.
// ---------------------------------------------------------------------------------------------
template <int MAXT, bool TAU = false>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? 3 : 1))
k_absorb_win(const AbsorbWinArgs A) {
  constexpr int NFC = WIN_NFC, NN = WIN_NODES, NH = WIN_NODES_H;
  static_assert(NN == NFC, "the node set is evaluated through the NFC-wide line bodies");
  static_assert(NFC == TAU_NFC, "tau rows are written in 16-frequency pieces");
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int64_t prof = blockIdx.x;
  const cmodel M = (cmodel)A.M;
  const cdoubles cfrq = (cdoubles)A.frq;
  typedef const __attribute__((address_space(4))) WinDesc* cwin;
  const cwin D = (cwin)(A.win + blockIdx.y);
  const cdoubles Lw = (cdoubles)(A.lagrange + (size_t)blockIdx.y * WIN_CHUNKS_MAX * NFC * NN);
  const cdoubles Lwh = (cdoubles)(A.lagrange_h + (size_t)blockIdx.y * WIN_CHUNKS_MAX * NFC * NH);
  __shared__ double sfn[3 * NFC + 2];                        // the nodes, laid out like a chunk
  __shared__ double sfn_h[3 * NH + 2];                       // the H2O nodes
  __shared__ double sfq_w[MAXT / WAVE][3 * NFC + 2];         // the current chunk, one copy per wave (fill_chunk_table)
  double* sfq = sfq_w[wave];
  if (tid < NN) {
    const double f = D->fnode[tid];
    sfn[2 * tid] = f; sfn[2 * tid + 1] = f * f; sfn[2 * NFC + 2 + tid] = 1.0;
  }
  if (tid >= NN && tid < NN + NH) {                          // (a one-wave workgroup has lanes 16 .. 23 too)
    const double f = D->fnode_h[tid - NN];
    sfn_h[2 * (tid - NN)] = f; sfn_h[2 * (tid - NN) + 1] = f * f; sfn_h[2 * NH + 2 + (tid - NN)] = 1.0;
  }
  if (tid == WAVE - 1) {                                     // cutoff / range votes at the nodes speak for the whole window
    sfn[2 * NFC] = D->flo; sfn[2 * NFC + 1] = D->fhi;
    sfn_h[2 * NH] = D->flo; sfn_h[2 * NH + 1] = D->fhi;
  }
  const int lev = TAU ? wave * (WAVE - 1) + lane : tid;
  const bool active = lev < A.nlev;
  const int64_t off = prof * A.nlev + (active ? lev : 0);
  const double pi = A.p[off], ti = A.t[off], rhi = A.rh[off];
  const int nch = D->nchunks;
  double zi = 0.0;
  bool bad = false;
  if constexpr (TAU) { zi = A.T.z[off]; bad = active && (isnan(zi) || isnan(pi) || isnan(ti) || isnan(rhi)); }
  if (__syncthreads_or(bad)) {                               // (also publishes sfn) check_for_nans: NaN out, valid = 0
    blank_tau(A.T, prof, A.nlev, D->first_chunk, nch, tid, blockDim.x);
    if (tid == 0) A.T.valid[prof] = 0;
    return;
  }
  const double e = goff_gratch_e(ti, rhi);
  const LevelState L = level_state(pi, ti, e);

  // ---- window-far lines at the nodes ----
  // The node sums live in LDS, [node][thread] (each lane reads back only its own column: conflict-free), not in
  // registers: 32 doubles per lane would cost the kernel two waves of occupancy.
  extern __shared__ __attribute__((aligned(16))) double wlds[];
  const int nthreads = blockDim.x;
  double* Sh_l = wlds;                                        // [NH][nthreads]
  double* So_l = wlds + (size_t)NH * nthreads;                // [NN][nthreads]
  const unsigned wf_both = D->h2o_far_both, wf_res = D->h2o_far_res;
  const unsigned long long wf_o2 = D->o2_far;
  double bsum_far = 0.0;
  unsigned failed_h = 0u;
  unsigned long long failed_o = 0ull;
  {
    LineMasks ln;
    ln.o2_far = wf_o2; ln.h2o_far = wf_both | wf_res; ln.h2o_res = wf_res; ln.h2o_none = 0u; ln.h2o_sd = 0u; ln.h2o_sdfar = 0u; ln.h2o_sdint = 0u;
    {
      double Sh[NH];
      h2o_absorb<NH, true>(M, L, sfn_h, ln, Sh, ~(wf_both | wf_res), nullptr, 0.0, &failed_h, &bsum_far);
#pragma unroll
      for (int m = 0; m < NH; ++m) Sh_l[m * nthreads + tid] = Sh[m];
    }
    double S[NN];
    dry_absorb<NFC, true>(M, L, sfn, ln, S, ~wf_o2, nullptr, &failed_o);
#pragma unroll
    for (int m = 0; m < NN; ++m) So_l[m * nthreads + tid] = S[m];
  }
  const unsigned excl_h = (wf_both | wf_res) & ~failed_h;     // a line that failed its vote at some level of this wave
  const unsigned long long excl_o = wf_o2 & ~failed_o;        // was left out of the node sums: evaluated directly
  // node sums -> a chunk's frequencies: out[j] = sum_m Lt[m][j] S[m]; the matrix is wave-uniform (scalar loads),
  // stored node-major so one node's 16 weights are one contiguous load
  auto interpolate = [&](const double* S_l, cdoubles Lt, int nn, double (&out)[NFC]) {
#pragma unroll
    for (int j = 0; j < NFC; ++j) out[j] = 0.0;
#pragma unroll 1
    for (int m = 0; m < nn; ++m) {                            // one node per trip: 16 scalar weights live at a time
      const double sm = S_l[m * nthreads + tid];
#pragma unroll
      for (int j = 0; j < NFC; ++j) out[j] = __builtin_fma((MWRT_ABLATE & 64) ? 0.0625 + 0.001 * j : Lt[m * NFC + j], sm, out[j]);
    }
  };

  // layer thickness below this level (TAU)
  bool has_prev = false, neg = false;
  double dz = 0.0;
  if constexpr (TAU) {
    has_prev = active && lev > 0 && lane > 0;
    const double z0 = A.T.z[prof * A.nlev];
    dz = has_prev ? ((zi - z0) - (A.T.z[off - 1] - z0)) : 0.0;
  }

  // ---- the window's chunks (no workgroup barrier inside: the waves drift apart and fill each other's stalls) ----
  for (int c = 0; c < nch; ++c) {
    const int jbase = (D->first_chunk + c) * NFC;
    const int nfc = min(NFC, A.nf - jbase);
    fill_chunk_table<NFC>(sfq, M, cfrq, jbase, nfc, lane);
    const cdoubles Lt = Lw + (size_t)c * NN * NFC;            // [node][target] of this chunk
    const cdoubles Lth = Lwh + (size_t)c * NH * NFC;
    const LineMasks lm = load_masks(A.masks, D->first_chunk + c);
    // The level state is the same for every chunk, and the compiler would hoist every per-(level, line) quantity
    // of the direct lines out of the chunk loop (hundreds of registers).  Laundering it keeps them inside.
    LevelState Lc = L;
    asm volatile("" : "+v"(Lc.t), "+v"(Lc.p), "+v"(Lc.rho), "+v"(Lc.pdry));
    double init[NFC], awet[NFC], adry[NFC];
    if constexpr (!TAU) {
      interpolate(Sh_l, Lth, NH, init);
      h2o_absorb<NFC>(M, Lc, sfq, lm, awet, excl_h, init, bsum_far, nullptr, nullptr,
                      (cdoubles)(A.lag_sd + (size_t)(D->first_chunk + c) * SD_TARGETS * SD_NODES));
      if (active) {
#pragma unroll
        for (int j = 0; j < NFC; ++j)
          if (j < nfc) A.awet[(prof * A.nf + jbase + j) * A.nlev + tid] = awet[j];
      }
      interpolate(So_l, Lt, NN, init);
      dry_absorb<NFC>(M, Lc, sfq, lm, adry, excl_o, init);
      if (active) {
#pragma unroll
        for (int j = 0; j < NFC; ++j)
          if (j < nfc) A.adry[(prof * A.nf + jbase + j) * A.nlev + tid] = adry[j];
      }
    } else {
      // One species is evaluated, run through the layer rule and PARKED (16 doubles) while the other is evaluated.
      // Wet first measured better than dry first on the real translation unit: 40 spilled VGPRs / 156 B of scratch per
      // lane against 52 / 212, and 3.70-3.77 against 3.83-3.93 ms on one box.
      auto layer_rows = [&](double (&x)[NFC]) {                // absorption -> layer optical depth of the layer below, in place
#pragma unroll
        for (int j = 0; j < NFC; j += 4) {
#pragma clang fp contract(off)
          double v4[4] = {x[j], x[j + 1], x[j + 2], x[j + 3]};
          const double vb[4] = {lane_below(v4[0]), lane_below(v4[1]), lane_below(v4[2]), lane_below(v4[3])};
          if (!(MWRT_ABLATE & 16)) layer_value4(v4, vb, neg, has_prev);
#pragma unroll
          for (int k = 0; k < 4; ++k) x[j + k] = has_prev ? v4[k] * dz : 0.0;
        }
      };
      interpolate(Sh_l, Lth, NH, init);
      h2o_absorb<NFC>(M, Lc, sfq, lm, awet, excl_h, init, bsum_far, nullptr, nullptr,
                      (cdoubles)(A.lag_sd + (size_t)(D->first_chunk + c) * SD_TARGETS * SD_NODES));
      layer_rows(awet);
      interpolate(So_l, Lt, NN, init);
      dry_absorb<NFC>(M, Lc, sfq, lm, adry, excl_o, init);
      layer_rows(adry);
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
#pragma clang fp contract(off)               // wet * dz + dry * dz rounds as in the fused kernel
        adry[j] = awet[j] + adry[j];
      }
      if (!((MWRT_ABLATE & 32) && adry[0] != -1.0)) {
        const int nlev = A.nlev;
        store_tau_chunk(adry, A.T.tau + prof * nlev * (int64_t)A.T.fpitch + jbase, A.T.fpitch, wave * (WAVE - 1), lane,
                        [&](int l, int ln) { return l < nlev && (ln > 0 || wave == 0); });
      }
    }
  }
  if constexpr (TAU) {
    if (__syncthreads_or(neg)) {                // pyrtlib raises ValueError here: flag 2, NaN out
      blank_tau(A.T, prof, A.nlev, D->first_chunk, nch, tid, nthreads);
      if (tid == 0) A.T.valid[prof] = 2;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K2 on fine spectral grids: downwelling Planck-space RTE (RTEquation.planck, from_sat = False, + bright [EXT]) from
// zenith layer optical depths in HBM, tau [nprof][nlev][fpitch] as the TAU absorption kernels write them.
//
// LANE = FREQUENCY.  A wave owns 64 consecutive frequencies of one profile and walks the levels serially: each step
// is one coalesced 512-byte row read (issued PF levels ahead), the Planck function of the level once per frequency,
// and the NA slant-path recursions in registers (B_a, T_a per elevation).  No LDS traffic in the loop (two
// broadcast reads of the level's h/kT), no barriers, no work split to recombine; thin or general layer step is voted
// per (level, elevation) by the wave -- neighbouring frequencies have neighbouring optical depths.
// Algorithmic traffic: 8 B per (profile, level, frequency) in, 8 B per TB out.
// ---------------------------------------------------------------------------------------------
constexpr int RTE_PF = 8;        // levels in flight per lane

template <int NA>
__global__ void __launch_bounds__(RTE_THREADS)
k_rte_tau(const RteTauArgs A) {
  extern __shared__ __attribute__((aligned(16))) double hkl[];    // {h/(k T_i) per GHz, its inverse} per level
  const int tid = threadIdx.x;
  const int64_t prof = blockIdx.x;
  const int nlev = A.nlev, nf = A.nf;
  const cmodel M = (cmodel)A.M;
  const cdoubles cam = (cdoubles)A.airmass;
  const double hk = 1e9 * M->planck_h / M->boltzmann_k;
  const double inv_hk = 1e-9 * M->boltzmann_k / M->planck_h;
  for (int l = tid; l < nlev; l += RTE_THREADS) {
    const double ti = A.t[prof * nlev + l];
    hkl[2 * l] = fdiv(hk, ti);
    hkl[2 * l + 1] = ti * inv_hk;
  }
  __syncthreads();
  const int f0 = blockIdx.y * RTE_THREADS + (tid & ~(WAVE - 1));
  if (f0 >= nf) return;                                           // a wave past the last frequency
  const int fi = blockIdx.y * RTE_THREADS + tid;
  const bool live = fi < nf;
  const int fc = live ? fi : nf - 1;                              // idle lanes shadow the last frequency (votes stay clean)
  const double qnan = __builtin_nan("");
  if (A.valid[prof] != 1) {                                       // NaN input / negative absorption: every TB of the profile is NaN
    if (live) {
#pragma unroll
      for (int a = 0; a < NA; ++a) A.tb[(prof * A.nang + A.a0 + a) * nf + fi] = qnan;
    }
    return;
  }
  const double f = A.frq[fc];
  const double rf = fdiv(1.0, f);
  double am[NA], B[NA], T[NA];
  double am_max = 0.0;                                            // NaN air masses (their rows come out NaN either way) aside
#pragma unroll
  for (int a = 0; a < NA; ++a) { am[a] = cam[A.a0 + a]; B[a] = 0.0; T[a] = 1.0; am_max = fmax(am_max, fabs(am[a])); }
  const double* col = A.tau + prof * nlev * (int64_t)A.fpitch + fc;
  const int64_t pitch = A.fpitch;
  double bprev = planck_b(f * hkl[0], rf * hkl[1]);
  double cur[RTE_PF];
#pragma unroll
  for (int k = 0; k < RTE_PF; ++k) cur[k] = col[(int64_t)min(1 + k, nlev - 1) * pitch];
  for (int i0 = 1; i0 < nlev; i0 += RTE_PF) {
    double nxt[RTE_PF];
#pragma unroll
    for (int k = 0; k < RTE_PF; ++k) nxt[k] = col[(int64_t)min(i0 + RTE_PF + k, nlev - 1) * pitch];
#pragma unroll
    for (int k = 0; k < RTE_PF; ++k) {
      const int i = i0 + k;
      if (i < nlev) {
        const double tz = cur[k];
        const double bi = planck_b(f * hkl[2 * i], rf * hkl[2 * i + 1]);
        // boflay (1 - E) = (B_{i-1} + B_i E) (1 - E)/(1 + E) = (B_{i-1} + B_i E) tanh(tau/2): the thin-layer step
        auto thin_step = [&](int a, double tl) {
          const double E = fexp_small(-tl);
          const double th = ftanh_half_small(tl);
          B[a] = __builtin_fma(__builtin_fma(bi, E, bprev) * T[a], th, B[a]);
          T[a] *= E;
        };
        if (wave_all(!(fabs(tz) * am_max > EXP_TINY_X))) {           // tiny at the longest path: the short series for every elevation
          KEEP_BRANCH();
#pragma unroll
          for (int a = 0; a < NA; ++a) {
            const double tl = tz * am[a];
            const double E = fexp_tiny(-tl);
            B[a] = __builtin_fma(__builtin_fma(bi, E, bprev) * T[a], ftanh_half_tiny(tl), B[a]);
            T[a] *= E;
          }
        } else if (wave_all(!(fabs(tz) * am_max > EXP_SMALL_X))) {   // thin at the longest path: thin at all of them, one vote
          KEEP_BRANCH();
#pragma unroll
          for (int a = 0; a < NA; ++a) thin_step(a, tz * am[a]);
        } else {
#pragma unroll
          for (int a = 0; a < NA; ++a) {
            const double tl = tz * am[a];
            if (wave_all(!(fabs(tl) > EXP_SMALL_X))) {
              thin_step(a, tl);
            } else {
              const double E = fexp(-tl);
              const double lay = fdiv1(__builtin_fma(bi, E, bprev), 1.0 + E);
              B[a] = __builtin_fma(lay * T[a], 1.0 - E, B[a]);
              T[a] *= E;
            }
          }
        }
        bprev = bi;
      }
    }
#pragma unroll
    for (int k = 0; k < RTE_PF; ++k) cur[k] = nxt[k];
  }
  if (!live) return;
  const double hvk = f * hk;
  const double bbg = fdiv(1.0, fexp(fdiv(hvk, M->t_cosmic)) - 1.0);   // B(T_cosmic, f)
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    // T is exp(-tauprof) of the whole path; pyrtlib's "tauprof < 125" cut is T > exp(-125)
    const double boftotl = (T[a] > TRANS_MIN) ? __builtin_fma(bbg, T[a], B[a]) : B[a];
    A.tb[(prof * A.nang + A.a0 + a) * nf + fi] = fdiv(hvk, flog(1.0 + fdiv(1.0, boftotl)));
  }
}

}  // namespace mwrt
