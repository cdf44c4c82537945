// mwrt_fused.hip.h -- the fused kernel (k_tb_fused) of the LBL forward operator, hand-written for gfx950 (CDNA4).
//
// Mapping: one workgroup = one (profile, frequency-chunk); one LANE = one LEVEL
// of that profile.  Line tables are wave-uniform and travel through the scalar unit (s_load),
// the chunk's frequencies are broadcast-read from LDS, and every per-(level,line) transcendental
// is evaluated once per lane and reused for the NFC frequencies of the chunk.  Phase K1 leaves zenith layer optical depths and
// Planck functions in LDS; phase K2 integrates the slant-path RTE out of LDS for all
// (frequency, angle) pairs; nothing but the 4 profile fields and the TBs touches HBM.
//
// Arithmetic restates pyrtlib [EXT] (not in /root/reference): RTEquation.vapor,
// clearsky_absorption -> H2OAbsModel.h2o_absorption / O2AbsModel.o2_absorption /
// N2AbsModel.n2_absorption, exponential_integration, planck, bright -- the routines that
// TbCloudRTE.execute() runs when called from reference python_src/proc/PyRTlib_processing.py:126.
// fp64 throughout ("dtype": "f64"); no MFMA: this is elementwise + scan work.
#pragma once
#include "mwrt_absorption.hip.h"
#include "mwrt_layer.hip.h"

namespace mwrt {

// ---------------------------------------------------------------------------------------------
// fused kernel: profile in -> TB out
// ---------------------------------------------------------------------------------------------
// NaN / negative-absorption exit: every output of this (profile, chunk) becomes NaN
__device__ __forceinline__ void blank_outputs(const FusedArgs& A, int64_t prof, int jbase, int nfc, int tid, int nthreads) {
  const double qnan = __builtin_nan("");
  const int nang = A.nang, nlev = A.nlev;
  for (int it = tid; it < nfc * nang; it += nthreads) {
    const int j = it / nang, a = it % nang;
    const int64_t o = (prof * nang + a) * A.nf + jbase + j;
    A.tb[o] = qnan;
    if (A.tbatm) A.tbatm[o] = qnan;
    if (A.tmr) A.tmr[o] = qnan;
    if (A.tauwet) A.tauwet[o] = qnan;
    if (A.taudry) A.taudry[o] = qnan;
    if (A.tauliq) A.tauliq[o] = qnan;
    if (A.tauice) A.tauice[o] = qnan;
  }
  if (A.taulay) for (int it = tid; it < nfc * nlev; it += nthreads)
    A.taulay[(prof * A.nf + jbase + it / nlev) * nlev + it % nlev] = qnan;
}

// The layers of one sorted K2 work item: `seglen` steps over tp[0 ..] / bp[0 ..] (zenith layer tau and B of the
// segment's levels).  The count is the same for every lane of the workgroup, so the loop runs on a scalar counter; a
// segment that ends past the top level reads the rows' zero padding there, and a layer of tau = 0 is an exact no-op
// (E = 1: T *= 1, B += x * 0).
// Four layers per trip, every value used in the registers it was loaded into: a pair of registers is reloaded only
// after its last use -- for a B value that is the step AFTER its own, which reads it as the level below -- so no
// copy carries anything round the loop; tau is in flight two steps ahead, B one and a half.  Each row is addressed
// from one LDS pointer that moves once per trip (opaque to the optimiser, which otherwise rebuilds base + offset
// every trip); the layers of a trip sit in the loads' immediate offsets.  The two layers loaded past the last one are
// dropped (they may lie beyond the zeroed part of the row: still inside the workgroup's LDS, see the row stride).
typedef const __attribute__((address_space(3))) double* ldoubles;
template <class Step>
__device__ __forceinline__ void rte_segment(const double* tau_seg, const double* bof_seg, int seglen, Step step) {
  ldoubles tp = (ldoubles)tau_seg, bp = (ldoubles)bof_seg;
  asm volatile("" : "+v"(tp), "+v"(bp));
  double t0 = tp[0], t1 = tp[1], b0 = bp[0], b1 = bp[1];
  for (int n = seglen >> 2; n > 0; --n) {
    const double t2 = tp[2], t3 = tp[3];
    step(t0, b0);
    const double b2 = bp[2], b3 = bp[3];
    step(t1, b1);
    t0 = tp[4]; t1 = tp[5];
    step(t2, b2);
    b0 = bp[4]; b1 = bp[5];
    step(t3, b3);
    tp += 4; bp += 4;
  }
  const int rest = seglen & 3;
  if (rest > 0) step(t0, b0);
  if (rest > 1) step(t1, b1);
  if (rest > 2) step(tp[2], bp[2]);
}

// NFC = frequencies per workgroup (accumulators in registers during K1);
// NFK = frequencies per K2 pass (rows of tau / B kept in LDS at a time): NFC = NPASS * NFK.
// Keeping only NFK rows resident holds the workgroup under 40 KB of LDS, so FOUR 192-thread
// workgroups (12 waves = 3 per SIMD) fit a CU and a 1000-profile batch is one resident round.
// (the TB-only variants are pinned to 3 waves per SIMD -- the clear-sky one sits at 161 of 168 VGPRs on its own and
// twelve more cost a third of the throughput; the cloud / ray-tracing one lands one register above the step and
// spills two; the RTE-from-absorption variant is pinned to the 4 waves its 256-thread launch relies on)
// (MWRT_MIN_WAVES, the pin of the EXTRAS variants: mwrt_math.hip.h)
// ALPHA = the K2 half alone: absorption coefficients are READ from HBM (what k_absorb wrote) instead of
// evaluated -- the two-kernel K1 -> alpha -> K2 form of the fine-grid configuration, and the entry for callers
// who bring their own absorption.
template <int NFC, int NFK, int MAXT, bool OPT = false, bool EXTRAS = false, bool ALPHA = false>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? (EXTRAS ? MWRT_MIN_WAVES : (ALPHA ? 4 : 3)) : 1))
k_tb_fused(const FusedArgs A) {
  constexpr int NPASS = (NFC + NFK - 1) / NFK;             // the last pass may hold fewer rows (14 = 8 + 6)
  static_assert(NPASS <= 2, "LaunchGeom carries the split of two passes");
  extern __shared__ __attribute__((aligned(16))) double lds[];     // 16-B base: wide ds_read stays aligned (guide G17)
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const int nthreads = blockDim.x;
  const int nwaves = nthreads / WAVE;
  const int64_t prof = blockIdx.x;                       // output row: model * nprof_in + profile
  const int mi = (int)(prof / A.nprof_in);
  const int64_t pin = prof - mi * A.nprof_in;            // input profile
  const int jbase = blockIdx.y * NFC;
  const int nfc = min(NFC, A.nf - jbase);
  const int nlev = A.nlev, nang = A.nang, ld = A.g.ldrow;
  const cmodel M = (cmodel)A.Ms[mi];
  const cdoubles cfrq = (cdoubles)A.frq;
  const cdoubles cam = (cdoubles)A.airmass;

  double* tau = lds;                                     // [NFK][ld] zenith layer optical depth (wet+dry)
  double* bof = tau + (size_t)NFK * ld;                  // [NFK][ld] Planck function B(T_i, f_j)
  double* part = bof + (size_t)NFK * ld;                 // [pairs*nseg][2] segment partials (B, T)
  double* scratch = part + (size_t)A.g.npart;            // [16] block_sum scratch
  double* edge = scratch + 16;                           // [nwaves][2*NFC] last lane of each wave
  // Until K2 fills them the tau / Planck rows are scratch, [frequency][level]: the wet absorption waits there while
  // dry_absorb runs, and the cloud block passes its liquid absorption through them.
  auto row = [&](int j) -> double* { return (j < NFK ? tau + (size_t)j * ld : bof + (size_t)(j - NFK) * ld); };
  // Parked wet sums and grouped far quads serve the 256- and 512-thread instantiations.  The 1024-thread ones (513 - 1024
  // levels) run under a 128-VGPR cap, where a group's N and D (56 registers more than the plain sums) go to scratch inside the
  // line loops: 600 levels took 260 us against 244, 1000 levels 366 against 340 (profiles/far_line_groups_ab.txt).  They keep
  // the quad form and the shuffle path.  No call can reach two MAXT with one profile, so every pair of instantiations that can
  // be compared bit for bit (TB-only, OPT, FULL, every chunk width) still shares one form.
  constexpr bool GROUPED = MAXT <= 512;
  constexpr bool PARK = !ALPHA && GROUPED;               // (ALPHA reads its coefficients just before the layer step)
  constexpr int GRP = 16;                                // levels per group of the layer-tau maxima
  const int ngrp = nthreads / GRP;
  float* gmax = (float*)(edge + (size_t)nwaves * 2 * NFC);   // [NFK][ngrp] largest zenith layer tau of 16 levels of a row
  int* wcnt = (int*)(gmax + (size_t)NFK * ngrp);          // [nwaves] thin work items per wave
  int* perm = wcnt + nwaves;                              // [nthreads] work items, thin ones first
  __shared__ int s_flag;
  __shared__ double sfq[5 * NFC + 2];                     // {f, f^2} per slot, {fmin, fmax}, N2 fdep, 1/f, cosmic-background Planck term per slot

  MWRT_STAMP(0);
#if MWRT_PHASE_CLOCK
  if (A.phase && lane == 0) {
    A.phase[((int64_t)blockIdx.x * 4 + wave) * 10 + 8] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
    A.phase[((int64_t)blockIdx.x * 4 + wave) * 10 + 9] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
  }
#endif
  // uniform frequency chunk; slots beyond nfc reuse the last valid one (results discarded)
  if (tid == 0) s_flag = 0;
  if (tid < NFC) {
    const double f = cfrq[jbase + min(tid, nfc - 1)];
    sfq[2 * tid] = f; sfq[2 * tid + 1] = f * f;
    double fdep = 1.0;
    if (M->n2_fdep) { const double q = f * (1.0 / 450.0); fdep = 0.5 + fdiv(0.5, 1.0 + q * q); }
    sfq[2 * NFC + 2 + tid] = fdep;
    sfq[3 * NFC + 2 + tid] = fdiv(1.0, f);
    // B(T_cosmic, f): one value per frequency, not per (frequency, angle) pair
    sfq[4 * NFC + 2 + tid] = fdiv(1.0, fexp(fdiv(f * (1e9 * M->planck_h / M->boltzmann_k), M->t_cosmic)) - 1.0);
  }
  if (tid == WAVE - 1) {
    double lo = cfrq[jbase], hi = lo;
    for (int j = 1; j < nfc; ++j) { const double f = cfrq[jbase + j]; lo = fmin(lo, f); hi = fmax(hi, f); }
    sfq[2 * NFC] = lo; sfq[2 * NFC + 1] = hi;
  }
  __syncthreads();

  const bool active = tid < nlev;
  // a wave beyond the top level (the RTE-from-absorption launch adds one for the K2 work items) holds no level:
  // it skips the per-level phases wave-uniformly and only meets the barriers
  const bool wave_live = wave * WAVE < nlev;
  const int64_t off = pin * nlev + (active ? tid : 0);
  double zi = A.z[off], ti = A.t[off];
  const double pi = ALPHA ? 0.0 : A.p[off], rhi = ALPHA ? 0.0 : A.rh[off];
  if (active && (isnan(zi) || isnan(pi) || isnan(ti) || isnan(rhi))) atomicOr(&s_flag, 1);
  double awet[NFC], adry[NFC];
  if constexpr (ALPHA) {
    bool bad = false;
    if (wave_live) {
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const int64_t o = (pin * A.nf + jbase + min(j, nfc - 1)) * nlev + (active ? tid : 0);     // 512-B rows per wave
        awet[j] = A.awet_in[o];
        adry[j] = A.adry_in[o];
        bad = bad || isnan(awet[j]) || isnan(adry[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < NFC; ++j) { awet[j] = 0.0; adry[j] = 0.0; }
    }
    if (active && bad) atomicOr(&s_flag, 1);
  }
  double denl = 0.0, deni = 0.0, o3n = 0.0;               // o3n: for the NaN test only, the ozone term reads it again
  if constexpr (OPT) {
    if (A.denliq) denl = A.denliq[off];
    if (A.denice) deni = A.denice[off];
    if (A.o3n) o3n = A.o3n[off];
    if (active && (isnan(denl) || isnan(deni) || isnan(o3n))) atomicOr(&s_flag, 1);
  }
  __syncthreads();
  if (s_flag) {                               // check_for_nans: outputs stay NaN, valid = 0
    blank_outputs(A, prof, jbase, nfc, tid, nthreads);
    if (tid == 0) A.valid[prof] = 0;
    return;
  }

  // ---- phase K1: absorption at my level for the NFC frequencies ----
  if constexpr (!ALPHA) {
    const double e = goff_gratch_e(ti, rhi);
    const LevelState L = level_state(pi, ti, e);
    const LineMasks lm = load_masks(A.masks[mi], blockIdx.y);
    MWRT_STAMP(1);
    MWRT_SETPRIO(3);
    h2o_absorb<NFC, false, GROUPED>(M, L, sfq, lm, awet);
    // the 14 wet sums would sit in 28 registers through the whole oxygen phase: they wait in LDS instead, and the layer
    // step reads its own and its lower neighbour's value from there (no crossbar, no wave seam for the wet half)
    if constexpr (PARK) {
      if (active) {
#pragma unroll
        for (int j = 0; j < NFC; ++j) row(j)[tid] = awet[j];
      }
    }
    MWRT_STAMP(2);
    MWRT_SETPRIO(2);
    dry_absorb<NFC, false, GROUPED>(M, L, sfq, lm, adry);
    MWRT_SETPRIO(1);
    MWRT_STAMP(3);
    if constexpr (OPT) {
      // The line loops need neither the ozone column nor z, T and p: they are read again where they are used (here and
      // after the barrier below) instead of riding through the line loops in registers -- the OPT variant sits at the
      // edge of its third wave.  (The fences keep the loads from being merged with the first ones.)
      if (A.o3n) {                                                 // clearsky_absorption(..., o3n): ozone joins the dry term
        LDS_RELOAD_FENCE();
        x_absorb<NFC>(M, A.t[off], A.p[off], A.o3n[off], sfq, adry);
      }
    }
  }
  // neighbour level i-1 of the dry half (and of the wet half where it is not parked): lane-1 through the crossbar,
  // wave seams through a 2*NFC-double edge row.  The barrier also orders the parking stores before the neighbour reads.
  if (lane == WAVE - 1) {
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
      if constexpr (!PARK) edge[wave * 2 * NFC + j] = awet[j];
      edge[wave * 2 * NFC + NFC + j] = adry[j];
    }
  }
  __syncthreads();
  if constexpr (OPT) { LDS_RELOAD_FENCE(); zi = A.z[off]; ti = A.t[off]; }
  // Wet and dry rows are kept apart only where the opacity columns are wanted (EXTRAS); otherwise td[] holds
  // the layer total (wet + dry, then + ice + liquid) and tw[] is never materialised: 28 registers fewer.
  double tw[EXTRAS ? NFC : 1], td[NFC];
  bool neg = false;
  {
    const double z0 = A.z[pin * nlev];        // execute() works in height above the antenna
    const double dz = (active && tid > 0) ? ((zi - z0) - (A.z[off - 1] - z0)) : 0.0;
    const bool seam = (lane == 0) && (wave > 0);
    const bool has_prev = active && tid > 0;
    // Parked wet sums: the rows are one block of LDS, row(j) = tau + j * ld, and a level's own value and its lower
    // neighbour's sit side by side, so every lane reads the pair at &row(j)[tid - 1] -- unconditionally (a lane without a
    // layer below it reads the first two entries of the row: it takes part in no vote and keeps no result), from one
    // pointer that moves a row per frequency, one frequency ahead of its use.
    [[maybe_unused]] ldoubles wrow = nullptr;
    [[maybe_unused]] double pw_next = 0.0, aw_next = 0.0;
    if constexpr (PARK) {
      wrow = (ldoubles)(tau + (has_prev ? tid - 1 : 0));
      asm volatile("" : "+v"(wrow));
      if (wave_live) { pw_next = wrow[0]; aw_next = wrow[1]; }
    }
    if (!wave_live) {
#pragma unroll
      for (int j = 0; j < NFC; ++j) { td[j] = 0.0; if constexpr (EXTRAS) tw[j] = 0.0; }
    } else
#pragma unroll
    for (int j = 0; j < NFC; ++j) {
#pragma clang fp contract(off)               // wet * dz + dry * dz rounds the same way in every instantiation
      double aw, pw;
      if constexpr (PARK) {
        aw = aw_next; pw = pw_next;
        if (j + 1 < NFC) { wrow += ld; pw_next = wrow[0]; aw_next = wrow[1]; }
      } else {
        aw = awet[j];
        pw = __shfl_up(awet[j], 1, WAVE);
        if (seam) pw = edge[(wave - 1) * 2 * NFC + j];
      }
      double pd = __shfl_up(adry[j], 1, WAVE);
      if (seam) pd = edge[(wave - 1) * 2 * NFC + NFC + j];
      const double lw = layer_value(aw, pw, neg, has_prev), ld_ = layer_value(adry[j], pd, neg, has_prev);
      const double twj = has_prev ? lw * dz : 0.0;
      const double tdj = has_prev ? ld_ * dz : 0.0;
      if constexpr (EXTRAS) { tw[j] = twj; td[j] = tdj; }
      else td[j] = twj + tdj;
    }
  }
  // cloud liquid / ice (opt-in): same layer rule with zeroflg = False; tau = ((wet + dry) + ice) + liquid
  // (kept as separate arrays only where the opacity columns are wanted; otherwise folded into the dry row)
  constexpr bool CLOUD_ROWS = OPT && EXTRAS;
  double tl[CLOUD_ROWS ? NFC : 1], tci[CLOUD_ROWS ? NFC : 1];
  if constexpr (OPT) {
#pragma unroll
    for (int j = 0; j < (CLOUD_ROWS ? NFC : 1); ++j) { tl[j] = 0.0; tci[j] = 0.0; }
    // Skipped when the profile holds no cloud at all (workgroup vote).  The liquid absorption of every level goes
    // through the tau / Planck rows of LDS, [frequency][level], so each lane reads its own and its
    // lower neighbour's value: no crossbar, no wave seams, and the per-level model state dies before the layer loop.
    // The vote is the barrier between the layer loop's reads of the parked wet sums and the stores below, which reuse
    // the same rows: no lane overwrites row(j)[tid] while lane tid + 1 still has to read it.
    const bool cloud_here = active && (denl > 0.0 || deni > 0.0);
    if ((A.denliq || A.denice) && __syncthreads_or(cloud_here)) {
      {
        const CloudLevel cl = cloud_level(M, ti);
        if (active) {
#pragma unroll
          for (int j = 0; j < NFC; ++j) row(j)[tid] = (denl > 0.0) ? liquid_abs(cl, sfq[2 * j], denl) : 0.0;
        }
      }
      __syncthreads();
      const bool has_below = active && tid > 0;
      const double deni_prev = (has_below && A.denice) ? A.denice[off - 1] : 0.0;
      const double z0 = A.z[pin * nlev];
      const double dz = has_below ? ((zi - z0) - (A.z[off - 1] - z0)) : 0.0;
#pragma unroll
      for (int j = 0; j < NFC; ++j) {
        const double f = sfq[2 * j];
        const double al = active ? row(j)[tid] : 0.0;
        const double pl = has_below ? row(j)[tid - 1] : 0.0;
        const double ai = (deni > 0.0) ? CLOUD_KICE * f * deni : 0.0;
        const double pc = (deni_prev > 0.0) ? CLOUD_KICE * f * deni_prev : 0.0;
        const double ll = layer_value<false>(al, pl, neg, has_below), li = layer_value<false>(ai, pc, neg, has_below);
        const double tlj = has_below ? ll * dz : 0.0;
        const double tij = has_below ? li * dz : 0.0;
        if constexpr (CLOUD_ROWS) { tl[j] = tlj; tci[j] = tij; }
        else td[j] = (td[j] + tij) + tlj;
      }
      __syncthreads();                          // the rows are about to be refilled with tau / B
    }
  }
  MWRT_STAMP(4);
  if (neg) atomicOr(&s_flag, 2);
  __syncthreads();
  if (s_flag) {                               // pyrtlib raises ValueError here: flag 2, NaN out
    blank_outputs(A, prof, jbase, nfc, tid, nthreads);
    if (tid == 0) A.valid[prof] = 2;
    return;
  }
  const double hk = 1e9 * M->planck_h / M->boltzmann_k;
  const double inv_hk = 1e-9 * M->boltzmann_k / M->planck_h;
  // The TB-only instantiation (EXTRAS = false) carries none of the by-product code: the compiler would
  // otherwise evaluate tbatm / tmr speculatively and keep the opacity sums' registers alive.
  bool want_tau = false;
  if constexpr (EXTRAS) {
    if (A.taulay && active) {
#pragma unroll
      for (int j = 0; j < NFC; ++j)
        if (j < nfc) {
          double tz = tw[j] + td[j];
          if constexpr (CLOUD_ROWS) tz = (tz + tci[j]) + tl[j];
          A.taulay[(prof * A.nf + jbase + j) * nlev + tid] = tz;
        }
    }
    want_tau = (A.tauwet != nullptr) || (A.taudry != nullptr) || (A.tauliq != nullptr) || (A.tauice != nullptr);
  }

  // The rows' padding, [nlev, ld), is zero in every row: a sorted pass runs each segment for its full length, and the
  // last one of a row ends there (rte_segment).  No pass writes these entries, so once is enough; the barrier that
  // every pass has between filling the rows and reading them orders these stores as well.
  for (int k = nlev + tid; k < ld; k += nthreads) {
#pragma unroll
    for (int jj = 0; jj < NFK; ++jj) { tau[jj * ld + k] = 0.0; bof[jj * ld + k] = 0.0; }
  }

  // ---- phase K2: slant-path RTE (RTEquation.planck, from_sat = False [EXT]), NFK rows at a time ----
#pragma unroll
  for (int h = 0; h < NPASS; ++h) {
    const int nfk = min(NFK, nfc - h * NFK);            // frequencies live in this pass (uniform)
    if (nfk <= 0) break;
    if (h > 0) MWRT_SETPRIO(0);
    if (h > 0) __syncthreads();                          // previous pass has finished reading LDS
    const int nseg = A.g.nseg[h], seglen = A.g.seglen[h];
    const int npairs = nfk * nang;
    const int items = (MWRT_ABLATE & 8) ? 0 : npairs * nseg;
    // wave-uniform: this pass deals its work items to the lanes thin ones first (see below)
    const bool sorted = !(OPT && A.amf) && items <= nthreads && seglen >= K2_SORT_MIN_SEGLEN;
    if (wave_live) {
      const double hkt = fdiv(hk, ti);                  // h / (k T) per GHz
      const double kth = ti * inv_hk;                   // its inverse, without a second division per lane
#pragma unroll
      for (int jj = 0; jj < NFK; ++jj) {
        const int j = h * NFK + jj;
        if (j < NFC) {
          double tz = td[j];
          if constexpr (EXTRAS) tz = tw[j] + td[j];
          if constexpr (CLOUD_ROWS) tz = (tz + tci[j]) + tl[j];
          const double bz = planck_b(sfq[2 * j] * hkt, sfq[3 * NFC + 2 + j] * kth);
          if (active) { tau[jj * ld + tid] = tz; bof[jj * ld + tid] = bz; }
          // largest layer value of each group of 16 levels (rounded up): decides once per work item whether
          // every layer of its segment is thin at its airmass
          if (sorted) {
            const float m = row16_max(active ? (float)tz * 1.0000005f : 0.0f);
            if ((lane & (GRP - 1)) == 0) gmax[jj * ngrp + tid / GRP] = m;
          }
        }
      }
    }
    // optional zenith opacity sums (tauwet / taudry columns); deterministic order
    double swet[EXTRAS ? NFK : 1], sdry[EXTRAS ? NFK : 1], sliq[EXTRAS ? NFK : 1], sice[EXTRAS ? NFK : 1];
    const bool rays = OPT && A.amf != nullptr;
    if constexpr (EXTRAS) {
      if (want_tau && !rays) {
#pragma unroll
        for (int jj = 0; jj < NFK; ++jj) {
          constexpr int JL = NFC - 1;
          const int j = min(h * NFK + jj, JL);               // rows past the chunk repeat the last one (never read)
          swet[jj] = block_sum(tw[j], scratch, tid, nthreads);
          sdry[jj] = block_sum(td[j], scratch, tid, nthreads);
          if constexpr (OPT) {
            sliq[jj] = block_sum(tl[j], scratch, tid, nthreads);
            sice[jj] = block_sum(tci[j], scratch, tid, nthreads);
          } else {
            sliq[jj] = 0.0; sice[jj] = 0.0;
          }
        }
      }
    }
    if constexpr (EXTRAS && OPT) {
      if (want_tau && rays) {
        // ray-traced paths: the opacity columns are sums of layer value x path factor, one species at a
        // time through the tau rows (the DataFrame path of a single execute(); not a throughput path)
        const int npairs_r = nfk * nang;
        for (int sp = 0; sp < 4; ++sp) {
          double* outp = sp == 0 ? A.tauwet : sp == 1 ? A.taudry : sp == 2 ? A.tauliq : A.tauice;
          __syncthreads();
          if (active) {
#pragma unroll
            for (int jj = 0; jj < NFK; ++jj) {
              const int j = h * NFK + jj;
              if (j < NFC) tau[jj * ld + tid] = sp == 0 ? tw[j] : sp == 1 ? td[j] : sp == 2 ? tl[j] : tci[j];
            }
          }
          __syncthreads();
          if (outp) for (int pr = tid; pr < npairs_r; pr += nthreads) {
            const int jj = pr / nang, a = pr - jj * nang;
            const double* fr = A.amf + (pin * nang + a) * nlev;
            double acc = 0.0;
            for (int i = 1; i < nlev; ++i) acc += tau[jj * ld + i] * fr[i];
            outp[(prof * nang + a) * A.nf + jbase + h * NFK + jj] = acc;
          }
        }
        __syncthreads();
        if (active) {
#pragma unroll
          for (int jj = 0; jj < NFK; ++jj) {
            const int j = h * NFK + jj;
            if (j < NFC) tau[jj * ld + tid] = ((tw[j] + td[j]) + tci[j]) + tl[j];
          }
        }
      }
    }
    __syncthreads();

    // Work item = (pair, level segment).  A layer is thin when tau * airmass <= 1/8: an item whose whole
    // segment is thin takes the division-free step.  The choice is per WAVE, so the items are dealt to the lanes
    // thin ones first (ballot ranks + one pass through LDS): at most one wave mixes both kinds and runs the
    // general step for all its lanes.  The maxima that decide it are per 16 levels of a row (gmax).
    int nthin_all = 0;
    if (sorted) {
      const bool mine = tid < items;
      const int it = mine ? tid : 0;
      const int pr = div_small(it, nseg, A.g.magic_nseg[h]), seg = it - pr * nseg;
      const int jj = div_small(pr, nang, A.g.magic_nang), a = pr - jj * nang;
      const int lo = 1 + seg * seglen, hi = min(lo + seglen, nlev);
      float gm = 0.0f;
      for (int g = lo / GRP; g <= (hi - 1) / GRP; ++g) gm = fmaxf(gm, gmax[jj * ngrp + g]);
      // a NaN airmass (its rows come out NaN either way) counts as thin
      const bool thin = mine && !((double)gm * cam[a] > EXP_SMALL_X);
      const unsigned long long bal = __ballot(thin);
      const int rank = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[wave] = __popcll(bal);
      __syncthreads();
      int before = 0, nthin = 0;
      for (int w = 0; w < nwaves; ++w) { const int c = wcnt[w]; nthin += c; if (w < wave) before += c; }
      if (mine) perm[thin ? before + rank : nthin + tid - (before + rank)] = (a << 11) | (jj << 7) | seg;
      nthin_all = nthin;
      __syncthreads();
    }
    for (int it0 = tid; it0 < items; it0 += nthreads) {
      int seg, jj, a;
      if (sorted) {
        const int key = perm[it0];
        seg = key & 127; jj = (key >> 7) & 15; a = key >> 11;
      } else {
        const int pr = div_small(it0, nseg, A.g.magic_nseg[h]);
        seg = it0 - pr * nseg; jj = div_small(pr, nang, A.g.magic_nang); a = pr - jj * nang;
      }
      const int it = (jj * nang + a) * nseg + seg;
      const double am = cam[a];
      const int lo = 1 + seg * seglen;
      const int hi = min(lo + seglen, nlev);
      const double* tj = tau + jj * ld;
      const double* bj = bof + jj * ld;
      const double* fr = nullptr;
      if constexpr (OPT) fr = A.amf ? A.amf + (pin * nang + a) * nlev : nullptr;
      double T = 1.0, B = 0.0;
      double bprev = (lo < nlev) ? bj[lo - 1] : 0.0;
      if (!sorted && !(OPT && fr) && nseg * seglen < ld) {
        // several rounds or short segments: thin or not is voted per step, by the lanes that hold an item -- a lane in
        // the zero padding past its last layer votes thin and changes no vote.  (This is the loop of the headline
        // shape: 56 pairs x 10 segments of 18 layers in three rounds, then 42 x 9 of 20 in two.)
        // A step voted thin runs the body of the sorted thin loop below -- tanh(tau/2) for (1 - E)/(1 + E), no division;
        // a padding lane (tau = 0) stays an exact no-op there as well: E = 1, th = 0.
        const double cs = loop_invariant_vgpr(FEXP_SMALL_C0), ce = loop_invariant_vgpr(FEXP_C0);
        const double ct = loop_invariant_vgpr(FTANH_HALF_SMALL_C0);
        // The steps work on -tau * airmass, formed with the negated air mass: both exponentials take it as it is, tanh is
        // odd and its sign goes into the last fma's source modifier -- no negation per step, the same bits.
        const double nam = -am;
        rte_segment(tj + lo, bj + lo, seglen, [&](double tz, double bi) {
          const double ntl = tz * nam;
          if (wave_all(fabs(ntl) <= EXP_SMALL_X)) {
            KEEP_BRANCH();
            const double E = fexp_small(ntl, cs);
            const double nth = ftanh_half_small(ntl, ct);
            B = __builtin_fma(__builtin_fma(bi, E, bprev) * T, -nth, B);
            T *= E;
          } else {
            KEEP_BRANCH();
            const double E = fexp(ntl, ce);
            const double lay = fdiv1(__builtin_fma(bi, E, bprev), 1.0 + E);
            B = __builtin_fma(lay * T, 1.0 - E, B);
            T *= E;
          }
          bprev = bi;
        });
      } else if (!sorted) {
        // ray-traced path factors (they vary with the level), or a row stride that stops short of nseg * seglen (segments
        // under K2_SORT_MIN_SEGLEN layers): each lane runs its own layers, thin or not is voted per step
        for (int i = lo; i < hi; ++i) {
          const double tl = tj[i] * ((OPT && fr) ? fr[i] : am);
          const double E = wave_all(fabs(tl) <= EXP_SMALL_X) ? fexp_small(-tl) : fexp(-tl);
          const double bi = bj[i];
          const double lay = fdiv1(__builtin_fma(bi, E, bprev), 1.0 + E);
          B = __builtin_fma(lay * T, 1.0 - E, B);
          T *= E;
          bprev = bi;
        }
      } else if (wave_all(it0 < nthin_all)) {
        // boflay (1 - E) = (B_{i-1} + B_i E) (1 - E)/(1 + E) = (B_{i-1} + B_i E) tanh(tau/2)
        const double ce = loop_invariant_vgpr(FEXP_SMALL_C0), ct = loop_invariant_vgpr(FTANH_HALF_SMALL_C0);
        rte_segment(tj + lo, bj + lo, seglen, [&](double tz, double bi) {
          const double tl = tz * am;
          const double E = fexp_small(-tl, ce);
          const double th = ftanh_half_small(tl, ct);
          B = __builtin_fma(__builtin_fma(bi, E, bprev) * T, th, B);
          T *= E;
          bprev = bi;
        });
      } else {
        const double ce = loop_invariant_vgpr(FEXP_C0);
        rte_segment(tj + lo, bj + lo, seglen, [&](double tz, double bi) {
          const double tl = tz * am;
          const double E = fexp(-tl, ce);
          const double lay = fdiv1(__builtin_fma(bi, E, bprev), 1.0 + E);
          B = __builtin_fma(lay * T, 1.0 - E, B);
          T *= E;
          bprev = bi;
        });
      }
      part[2 * it + 0] = B; part[2 * it + 1] = T;
    }
    MWRT_STAMP(5 + h);
    __syncthreads();
    for (int pr = tid; pr < npairs; pr += nthreads) {
      const int jj = div_small(pr, nang, A.g.magic_nang);
      const int a = pr - jj * nang;
      const int j = h * NFK + jj;
      double B = 0.0, T = 1.0;
      for (int sg = 0; sg < nseg; ++sg) {
        const double* q = part + 2 * (pr * nseg + sg);
        B = __builtin_fma(T, q[0], B);
        T *= q[1];
      }
      const double hvk = cfrq[jbase + j] * hk;
      double boftotl, boftmr;
      // T is exp(-tauprof) of the whole path; pyrtlib's "tauprof < 125" cut is T > exp(-125) (beyond it the
      // cosmic term is 1e-54 of B either way)
      if (T > TRANS_MIN) {
        const double ex = T;
        const double bbg = sfq[4 * NFC + 2 + j];
        boftotl = __builtin_fma(bbg, ex, B);
        boftmr = EXTRAS ? fdiv(B, 1.0 - ex) : 0.0;
      } else {
        boftotl = B; boftmr = B;
      }
      const int64_t o = (prof * nang + a) * A.nf + jbase + j;
      A.tb[o] = fdiv(hvk, flog(1.0 + fdiv(1.0, boftotl)));
      if constexpr (EXTRAS) {
        if (A.tbatm) A.tbatm[o] = fdiv(hvk, flog(1.0 + fdiv(1.0, B)));
        if (A.tmr) A.tmr[o] = fdiv(hvk, flog(1.0 + fdiv(1.0, boftmr)));
        if (want_tau && !rays) {
          const double am = cam[a];
          double sw = 0.0, sd = 0.0, sl = 0.0, si = 0.0;
#pragma unroll
          for (int q2 = 0; q2 < NFK; ++q2) if (q2 == jj) { sw = swet[q2]; sd = sdry[q2]; sl = sliq[q2]; si = sice[q2]; }
          if (A.tauwet) A.tauwet[o] = sw * am;
          if (A.taudry) A.taudry[o] = sd * am;
          if (A.tauliq) A.tauliq[o] = sl * am;
          if (A.tauice) A.tauice[o] = si * am;
        }
      }
    }
  }
  if constexpr (OPT) {
    // a trapped ray (ducting) leaves its angle NaN and marks the profile 3
    if (A.duct && A.duct[pin]) { if (tid == 0) A.valid[prof] = 3; return; }
  }
  if (A.write_valid && tid == 0) A.valid[prof] = 1;
  MWRT_STAMP(7);
}

}  // namespace mwrt
