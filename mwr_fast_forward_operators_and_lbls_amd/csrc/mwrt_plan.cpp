// mwrt_plan.cpp -- the host's launch planning (declarations: mwrt_plan.h).  No HIP in here.
#include "mwrt_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace mwrt {

namespace {

// K2 work split: items = pairs x nseg over `threads` lanes; cost ~ rounds x seglen (+ combine)
// segments per (frequency, angle) pair for one K2 pass of `npairs` pairs: fill the workgroup in one round
int plan_k2_pass(int nlev, int npairs, int threads) {
  const int layers = nlev - 1;
  int best = 1; long best_cost = -1;
  for (int ns = 1; ns <= 64 && ns <= (layers > 0 ? layers : 1); ++ns) {
    const int sl = (layers + ns - 1) / ns;
    const long rounds = ((long)npairs * ns + threads - 1) / threads;
    const long cost = rounds * (sl * 8L + 4) + ns;      // 8 ~ relative cost of a layer step vs a combine step
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ns; }
  }
  return best;
}

// rows of the two K2 passes of a chunk
int rows0_of(int nfc, int nf) { return std::min(NFK, std::min(nfc, nf)); }
int rows1_of(int nfc, int nf) { return std::max(0, std::min(nfc, nf) - NFK); }

void set_pass(LaunchGeom* g, int h, int nlev, int ns) {
  g->nseg[h] = ns < 1 ? 1 : ns;
  g->seglen[h] = (nlev - 1 + g->nseg[h] - 1) / g->nseg[h];
  if (g->seglen[h] < 1) g->seglen[h] = 1;
}

// the geometry that follows from the segment counts of the two passes
void set_split(LaunchGeom* g, int nlev, int nfc, int nf, int nang, int ns0, int ns1) {
  set_pass(g, 0, nlev, ns0);
  set_pass(g, 1, nlev, ns1);
  g->npart = 2 * nang * std::max(rows0_of(nfc, nf) * g->nseg[0], rows1_of(nfc, nf) * g->nseg[1]);
  g->magic_nseg[0] = magic_of(g->nseg[0]);
  g->magic_nseg[1] = magic_of(g->nseg[1]);
  g->magic_nang = magic_of(nang);
  // Row stride in doubles.  A pass that deals its items out sorted (seglen >= K2_SORT_MIN_SEGLEN) runs every segment for
  // the full seglen layers, so the last segment of a row reads up to index nseg * seglen: the row reaches that far, and
  // the kernel zero-fills it from nlev on (a layer of tau = 0 leaves B and T as they are).  An odd multiple of 2 dwords
  // keeps ds_read_b64 rows on distinct banks.
  int ld = nlev + 1;
  for (int h = 0; h < 2; ++h)
    if (g->seglen[h] >= K2_SORT_MIN_SEGLEN) ld = std::max(ld, g->nseg[h] * g->seglen[h] + 1);
  if ((ld & 1) == 0) ld += 1;
  g->ldrow = ld;
}

LaunchGeom plan_k2(int nlev, int nfc, int nf, int nang, int threads) {
  LaunchGeom g;
  const int rows1 = rows1_of(nfc, nf);
  set_split(&g, nlev, nfc, nf, nang, plan_k2_pass(nlev, rows0_of(nfc, nf) * nang, threads),
            rows1 > 0 ? plan_k2_pass(nlev, rows1 * nang, threads) : 1);
  return g;
}

size_t fused_lds_bytes(int nfc, const LaunchGeom& g, int threads) {
  // float gmax[NFK][threads/16], int wcnt[nwaves], int perm[threads]
  const size_t sort_doubles = ((size_t)NFK * (threads / 16) + (threads / WAVE) + threads + 1) / 2;
  return sizeof(double) * ((size_t)2 * NFK * g.ldrow + (size_t)g.npart + 16 +
                           (size_t)(threads / WAVE) * 2 * nfc + sort_doubles);
}

// upper bound of a speed-dependent H2O line's half width anywhere in an atmosphere (dry air <= 1100 hPa, vapour
// <= 150 hPa, T >= 148 K): the host may put such a line in a window's far set only where 10 half-widths cannot
// reach the window; the kernel re-checks per level and takes the line back if they can
double sd_halfwidth_bound(const mwrt_model_desc& t, int k) {
  return t.h2o_w0[k] * 1100.0 * std::pow(2.0, std::max(t.h2o_x[k], 0.0)) +
         t.h2o_w0s[k] * 150.0 * std::pow(2.0, std::max(t.h2o_xs[k], 0.0));
}

// Chebyshev nodes of [flo, fhi] and the barycentric Lagrange weights of every target frequency of the window,
// stored [chunk][node][target]; targets past the last frequency repeat it (their results are discarded)
template <int NNODES>
void window_nodes(const double* frq, int b, int e, int nchunks, double* fnode, double* blk_base) {
  const int per = nchunks * WIN_NFC;
  const double flo = frq[b], fhi = frq[e];
  long double x[NNODES], bw[NNODES];
  for (int m = 0; m < NNODES; ++m)
    fnode[m] = (double)(0.5L * (flo + fhi) + 0.5L * (fhi - flo) * cosl(M_PIl * (2 * m + 1) / (2.0L * NNODES)));
  for (int m = 0; m < NNODES; ++m) x[m] = fnode[m];                // weights for the nodes as the kernel sees them
  for (int m = 0; m < NNODES; ++m) {
    long double prod = 1.0L;
    for (int k = 0; k < NNODES; ++k) if (k != m) prod *= (x[m] - x[k]);
    bw[m] = 1.0L / prod;
  }
  for (int r = 0; r < per; ++r) {
    const long double f = frq[std::min(b + r, e)];
    const int cidx = r / WIN_NFC, j = r % WIN_NFC;
    double* blk = blk_base + (size_t)cidx * NNODES * WIN_NFC;
    int hit = -1;
    for (int m = 0; m < NNODES; ++m) if (f == x[m]) hit = m;
    if (hit >= 0) { blk[hit * WIN_NFC + j] = 1.0; continue; }
    long double q[NNODES], sum = 0.0L;
    for (int m = 0; m < NNODES; ++m) { q[m] = bw[m] / (f - x[m]); sum += q[m]; }
    for (int m = 0; m < NNODES; ++m) blk[m * WIN_NFC + j] = (double)(q[m] / sum);
  }
}

// far-line sets of a window [flo, fhi]: an O2 line is far beyond max(4 GHz, 1.6 half-spans), an H2O line beyond
// max(30 GHz, 11.8 half-spans) -- the distance-to-half-span ratios the 16- and 8-node interpolations were sized for
void window_far_sets(const mwrt_model_desc& t, double flo, double fhi, WinDesc* d) {
  const double half = 0.5 * (fhi - flo);
  const double mo = std::max(WIN_MARGIN_GHZ, 1.6 * half), mh = std::max(WIN_H2O_MARGIN_GHZ, 11.8 * half);
  d->o2_far = 0; d->h2o_far_both = 0; d->h2o_far_res = 0;
  for (int k = 0; k < t.n_o2; ++k) {
    const double c = t.o2_f[k];
    if (c < flo - mo || c > fhi + mo) d->o2_far |= 1ull << k;
  }
  for (int k = 0; k < t.n_h2o; ++k) {
    const double c = t.h2o_fl[k];
    if (!(c < flo - mh || c > fhi + mh)) continue;
    // a speed-dependent line stays direct wherever its special shape (inside 10 half-widths) could reach the window
    if (t.h2o_w2[k] > 0.0 && !(10.0 * sd_halfwidth_bound(t, k) < std::min(std::fabs(c - flo), std::fabs(c - fhi)) - 1.0)) continue;
    const double g = WIN_CUTOFF_GUARD_GHZ;
    const bool d1_in = std::fabs(flo - c) < 750.0 - g && std::fabs(fhi - c) < 750.0 - g;
    const bool d2_in = fhi + c < 750.0 - g;
    const bool d2_out = flo + c >= 750.0 + g;
    if (d1_in && d2_in) d->h2o_far_both |= 1u << k;
    else if (d1_in && d2_out) d->h2o_far_res |= 1u << k;
    // anything else (a cutoff crossing the window, or both terms out) is left to the per-chunk loops
  }
}

// Lagrange weights of the half-sampled speed-dependent shape for one full chunk f[0 .. 15]: w[target][node], the odd slots
// from slots 0, 2, ..., 14, 15 (w may be null).  False where the chunk cannot be half-sampled: frequencies not increasing,
// or some target's weights sum to more than SD_LEBESGUE_MAX in absolute value (near-coincident frequencies next to a gap).
bool sd_half_weights(const double* f, double* w) {
  for (int j = 1; j < WIN_NFC; ++j) if (!(f[j] > f[j - 1])) return false;
  bool ok = true;
  for (int i = 0; i < SD_TARGETS; ++i) {
    const long double x = f[2 * i + 1];
    long double lebesgue = 0.0L;
    for (int n = 0; n < SD_NODES; ++n) {
      long double wn = 1.0L;
      for (int q = 0; q < SD_NODES; ++q)
        if (q != n) wn *= (x - (long double)f[sd_node_slot(q)]) / ((long double)f[sd_node_slot(n)] - (long double)f[sd_node_slot(q)]);
      lebesgue += fabsl(wn);
      if (w) w[i * SD_NODES + n] = (double)wn;
    }
    if (!(lebesgue <= SD_LEBESGUE_MAX)) ok = false;
  }
  return ok;
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

unsigned magic_of(int d) { return d <= 1 ? 0u : (unsigned)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d); }

bool plan_fused(int lds_max, int nfc, int nlev, int nf, int nang, LaunchGeom* g, size_t* lds, int threads) {
  if (threads <= 0) threads = lanes_for(nlev);
  *g = plan_k2(nlev, nfc, nf, nang, threads);
  *lds = fused_lds_bytes(nfc, *g, threads);
  while (*lds > (size_t)lds_max && (g->nseg[0] > 1 || g->nseg[1] > 1)) {     // shrink the partials if LDS is short
    set_split(g, nlev, nfc, nf, nang, (g->nseg[0] + 1) / 2, (g->nseg[1] + 1) / 2);
    *lds = fused_lds_bytes(nfc, *g, threads);
  }
  return *lds <= (size_t)lds_max;
}

// frequency-chunk width: 14 HATPRO channels fit one chunk exactly; other counts use 16 / 8
int pick_nfc(int nf) {
  if (nf % 14 == 0 || nf <= 14) return (nf <= 8) ? 8 : 14;
  return 16;
}

// ... unless the caller fixed the width (mwrt_set_chunk_width: 8 splits a 14-channel profile over two workgroups, each with
// the full per-(level, line) set-up but half the line-frequency work -- one profile 58 instead of 75 us, 256 profiles 61
// instead of 76, 512 profiles 77 instead of 83 at seven elevations; not the default because results would then depend, in the
// 13th digit, on how a caller batches its profiles) or the profile is so tall that the wide chunk's LDS rows do not fit: then 8
int pick_nfc_fused(int chunk_width, int lds_max, int nlev, int nf, int nang) {
  int nfc = chunk_width ? chunk_width : pick_nfc(nf);
  LaunchGeom g; size_t lds;
  if (!plan_fused(lds_max, nfc, nlev, nf, nang, &g, &lds)) nfc = 8;
  return nfc;
}

bool any_nan(const double* x, int n) {
  for (int i = 0; i < n; ++i) if (std::isnan(x[i])) return true;
  return false;
}

bool all_nan(const double* x, int n) {
  for (int i = 0; i < n; ++i) if (!std::isnan(x[i])) return false;
  return true;
}

// (NaN elevation -> NaN air mass: that angle's rows come out NaN)
bool airmass_of(const double* elev, int nang, std::vector<double>* am) {
  am->resize(nang);
  for (int a = 0; a < nang; ++a) {
    // The wrapper tests ang = [elevation_k] per k (PyRTlib_processing.py:106, :117) and skips only that
    // k: a NaN elevation blanks its own [:, k, :] rows and nothing else.  Its air mass is NaN, which
    // the slant-path integration carries into every output of that angle; valid[] is about the
    // profile's own data and stays 1.
    if (std::isnan(elev[a])) { (*am)[a] = std::nan(""); continue; }
    // a path at or below the horizon has no plane-parallel air mass
    if (!(elev[a] > 0.0 && elev[a] < 180.0)) return false;
    (*am)[a] = 1.0 / std::sin(elev[a] * M_PI / 180.0);
  }
  return true;
}

int rte_tau_angles(int rem) { return rem <= 8 ? rem : (rem == 10 ? 10 : (rem == 9 ? 5 : 8)); }

// ---- fine-grid two-kernel form: K1 + layer step -> zenith layer optical depth in HBM -> RTE ----
int tau_pitch_of(int nf) { return ((nf + TAU_NFC - 1) / TAU_NFC) * TAU_NFC; }

size_t absorb_win_lds_bytes(int threads) {
  const int maxt = threads <= 256 ? 256 : 512;
  return sizeof(double) * ((size_t)(WIN_NODES + WIN_NODES_H) * threads + (3 * WIN_NFC + 2) * (1 + maxt / WAVE) +
                           (3 * WIN_NODES_H + 2)) + 64;
}

bool windows_eligible(const double* frq, int nf) {
  if (nf < WIN_CHUNKS * WIN_NFC) return false;
  for (int j = 1; j < nf; ++j) if (!(frq[j] > frq[j - 1])) return false;
  const int per = WIN_CHUNKS * WIN_NFC;
  for (int b = 0; b < nf; b += per) {
    const int e = std::min(nf, b + per) - 1;
    if (e == b) return false;                              // a one-frequency window has no span to put nodes on
    if (frq[e] - frq[b] > WIN_MAX_SPAN_GHZ) return false;
  }
  return true;
}

AbsorbRoute absorption_route(int mode, int lds_max, const double* frq, int nf, int threads) {
  // can the windowed absorption kernel serve this call (frequency list, level count, LDS)?
  const bool ok = windows_eligible(frq, nf) && threads <= 512 && absorb_win_lds_bytes(threads) <= (size_t)lds_max;
  if (mode == 2 && !ok) return AbsorbRoute::refused;
  return ok && mode != 1 ? AbsorbRoute::windowed : AbsorbRoute::every_line;
}

void chunk_masks(const mwrt_model_desc& t, const double* frq, int nf, int nfc, std::vector<LineMasks>* out) {
  const int nchunks = (nf + nfc - 1) / nfc;
  out->assign(nchunks, LineMasks{});
  for (int ch = 0; ch < nchunks; ++ch) {
    const int j0 = ch * nfc, j1 = std::min(nf, j0 + nfc);
    LineMasks& lm = (*out)[ch];
    // very far lines (vfar_add): poles of the line's term in u = f^2, u ~ c^2 -+ 2 i c w, at >= 1/VF_RATIO_MAX half ranges
    // from the middle of the chunk's f^2 values -- with 2 GHz of allowance for pressure shifts and 10 GHz for the half width
    double ulo = 1e300, uhi = 0.0;
    for (int j = j0; j < j1; ++j) { ulo = std::min(ulo, frq[j] * frq[j]); uhi = std::max(uhi, frq[j] * frq[j]); }
    lm.vf_u0 = 0.5 * (ulo + uhi);
    lm.vf_h = std::max(0.5 * (uhi - ulo), 1.0);
    lm.vf_invh = 1.0 / lm.vf_h;
    auto very_far = [&](double c) {
      const double cl = std::max(c - 2.0, 0.0), ch = c + 2.0;
      const double plo = cl * cl - 100.0, phi = ch * ch;             // real part of the poles lies in [plo, phi]
      const double dist = (lm.vf_u0 < plo) ? plo - lm.vf_u0 : ((lm.vf_u0 > phi) ? lm.vf_u0 - phi : 0.0);
      return lm.vf_h <= VF_RATIO_MAX * dist;
    };
    // (a line costs ~40 instructions in the polynomial against 7 per frequency directly: not worth it under 7 frequencies)
    static const bool no_vfar_env = std::getenv("MWRT_NO_VFAR") != nullptr;               // diagnostic: time the direct sums
    const bool no_vfar = no_vfar_env || (j1 - j0) < VF_MIN_FREQS;
    for (int k = 0; k < t.n_o2; ++k) {
      double dmin = 1e300;
      for (int j = j0; j < j1; ++j) dmin = std::min(dmin, std::fabs(frq[j] - t.o2_f[k]));
      if (dmin >= FAR_MIN_GHZ + FAR_SHIFT_GHZ) lm.o2_far |= 1ull << k;
      if (!no_vfar && very_far(t.o2_f[k])) lm.o2_vfar |= 1ull << k;
    }
    if (__builtin_popcountll(lm.o2_vfar) < VF_MIN_LINES) lm.o2_vfar = 0;
    // half-sampled shape: a full 16-frequency chunk of increasing frequencies whose slots interpolate stably ...
    const bool half_ok = nfc == 16 && j1 - j0 == 16 && sd_half_weights(frq + j0, nullptr);
    for (int k = 0; k < t.n_h2o; ++k) {
      double dmin = 1e300, smin = 1e300;
      for (int j = j0; j < j1; ++j) { dmin = std::min(dmin, std::fabs(frq[j] - t.h2o_fl[k])); smin = std::min(smin, std::fabs(frq[j] + t.h2o_fl[k])); }
      if (dmin >= FAR_H2O_GHZ) lm.h2o_far |= 1u << k;
      if (!no_vfar && very_far(t.h2o_fl[k])) lm.h2o_vfar |= 1u << k;
      if (dmin >= 750.0 + FAR_H2O_GHZ && smin >= 750.0 + FAR_H2O_GHZ) lm.h2o_none |= 1u << k;
      if (smin >= 750.0 + FAR_H2O_GHZ) lm.h2o_res |= 1u << k;
      if (t.h2o_w2[k] > 0.0) {
        lm.h2o_sd |= 1u << k;
        if (10.0 * sd_halfwidth_bound(t, k) < dmin - 1.0) lm.h2o_sdfar |= 1u << k;       // its special shape cannot reach the chunk
        // ... >= 3 GHz and 5 spans from the centre
        static const bool no_half = std::getenv("MWRT_NO_SD_HALF") != nullptr;            // diagnostic: time the full sampling
        if (half_ok && !no_half && dmin >= 3.0 && dmin >= 5.0 * (frq[j1 - 1] - frq[j0])) lm.h2o_sdint |= 1u << k;
      }
    }
    if (__builtin_popcount(lm.h2o_vfar) < VF_MIN_LINES) lm.h2o_vfar = 0;
  }
}

void build_windows(const mwrt_model_desc& t, const double* frq, int nf, WindowSet* ws) {
  const int per = WIN_CHUNKS * WIN_NFC;
  const int nchunks = (nf + WIN_NFC - 1) / WIN_NFC;
  const int nbase = (nf + per - 1) / per;
  // base windows of WIN_CHUNKS chunks; two neighbours are MERGED (one node phase for both) when the merged window
  // keeps every O2 line far and loses no H2O line from the far set: the out-of-band stretches of a spectrum
  struct Span { int c0, nch; };
  std::vector<Span> spans;
  auto bounds = [&](const Span& sp, int* b, int* e) { *b = sp.c0 * WIN_NFC; *e = std::min(nf, (sp.c0 + sp.nch) * WIN_NFC) - 1; };
  for (int w = 0; w < nbase; ++w) spans.push_back({w * WIN_CHUNKS, std::min(WIN_CHUNKS, nchunks - w * WIN_CHUNKS)});
  const bool merge = std::getenv("MWRT_WIN_NOMERGE") == nullptr;                       // diagnostic: time the unmerged windows
  for (size_t i = 0; i + 1 < spans.size();) {
    const Span m{spans[i].c0, spans[i].nch + spans[i + 1].nch};
    bool ok = merge && spans[i].nch == WIN_CHUNKS && m.nch <= WIN_CHUNKS_MAX;
    if (ok) {
      int b, e; bounds(m, &b, &e);
      WinDesc dm{}, d0{}, d1{};
      window_far_sets(t, frq[b], frq[e], &dm);
      int b0, e0, b1, e1; bounds(spans[i], &b0, &e0); bounds(spans[i + 1], &b1, &e1);
      window_far_sets(t, frq[b0], frq[e0], &d0);
      window_far_sets(t, frq[b1], frq[e1], &d1);
      const unsigned long long all_o2 = t.n_o2 >= 64 ? ~0ull : ((1ull << t.n_o2) - 1ull);
      ok = dm.o2_far == all_o2 &&                                                     // no O2 line anywhere near
           (dm.h2o_far_both | dm.h2o_far_res) == ((d0.h2o_far_both | d0.h2o_far_res) & (d1.h2o_far_both | d1.h2o_far_res));
    }
    if (ok) { spans[i] = m; spans.erase(spans.begin() + (long)i + 1); ++i; }           // (a merged window is not merged again)
    else ++i;
  }
  // Workgroups are dispatched in grid order (profiles fastest, then windows): the EXPENSIVE windows go first, so that the
  // last, partly filled round of the launch is made of cheap ones (the oxygen band sits at the end of a 20-60 GHz grid).
  // Cost per frequency, roughly, in instructions: a floor, 12 per oxygen line evaluated directly, the speed-dependent shape
  // where some level can be inside its 10 half-widths.
  if (std::getenv("MWRT_WIN_GRID_ORDER") == nullptr) {                                   // (diagnostic: keep the grid order)
    auto cost = [&](const Span& sp) {
      int b, e; bounds(sp, &b, &e);
      WinDesc d{};
      window_far_sets(t, frq[b], frq[e], &d);
      const unsigned long long all_o2 = t.n_o2 >= 64 ? ~0ull : ((1ull << t.n_o2) - 1ull);
      double per_f = 150.0 + 12.0 * __builtin_popcountll(~d.o2_far & all_o2);
      for (int k = 0; k < t.n_h2o; ++k) {
        if (!(t.h2o_w2[k] > 0.0)) continue;
        const double c = t.h2o_fl[k];
        const double dist = (c < frq[b]) ? frq[b] - c : ((c > frq[e]) ? c - frq[e] : 0.0);
        per_f += 50.0 * std::max(0.0, 1.0 - dist / (10.0 * sd_halfwidth_bound(t, k)));
      }
      return per_f * (e - b + 1);
    };
    std::stable_sort(spans.begin(), spans.end(), [&](const Span& x, const Span& y) { return cost(x) > cost(y); });
  }
  // Lagrange weights of the half-sampled speed-dependent shape, per chunk (zero for a partial last chunk and for a chunk
  // that chunk_masks never half-samples: never used)
  ws->lag_sd.assign((size_t)nchunks * SD_TARGETS * SD_NODES, 0.0);
  for (int ch = 0; ch < nchunks; ++ch) {
    if ((ch + 1) * WIN_NFC > nf) continue;
    double w[SD_TARGETS * SD_NODES];
    if (sd_half_weights(frq + (size_t)ch * WIN_NFC, w)) std::copy(w, w + SD_TARGETS * SD_NODES, ws->lag_sd.begin() + (size_t)ch * SD_TARGETS * SD_NODES);
  }
  const int nwin = (int)spans.size();
  const int perm = WIN_CHUNKS_MAX * WIN_NFC;
  ws->wins.assign(nwin, WinDesc{});
  ws->lag.assign((size_t)nwin * perm * WIN_NODES, 0.0);
  ws->lag_h.assign((size_t)nwin * perm * WIN_NODES_H, 0.0);
  for (int w = 0; w < nwin; ++w) {
    WinDesc& d = ws->wins[w];
    int b, e; bounds(spans[w], &b, &e);
    d.flo = frq[b]; d.fhi = frq[e];
    d.first_chunk = spans[w].c0;
    d.nchunks = spans[w].nch;
    window_nodes<WIN_NODES>(frq, b, e, d.nchunks, d.fnode, ws->lag.data() + (size_t)w * perm * WIN_NODES);
    window_nodes<WIN_NODES_H>(frq, b, e, d.nchunks, d.fnode_h, ws->lag_h.data() + (size_t)w * perm * WIN_NODES_H);
    window_far_sets(t, d.flo, d.fhi, &d);
  }
}

WindowLayout window_layout(int nwin, int nf) {
  const size_t perm = (size_t)WIN_CHUNKS_MAX * WIN_NFC, nchunks = (size_t)(nf + WIN_NFC - 1) / WIN_NFC;
  WindowLayout l;
  l.off_lag = up256(sizeof(WinDesc) * (size_t)nwin);
  l.off_lagh = l.off_lag + up256(sizeof(double) * (size_t)nwin * perm * WIN_NODES);
  l.off_lagsd = l.off_lagh + up256(sizeof(double) * (size_t)nwin * perm * WIN_NODES_H);
  l.total = l.off_lagsd + up256(sizeof(double) * nchunks * SD_TARGETS * SD_NODES);
  return l;
}

void pack_windows(const WindowSet& ws, int nf, std::vector<char>* blob) {
  const WindowLayout l = window_layout((int)ws.wins.size(), nf);
  blob->assign(l.total, 0);
  std::memcpy(blob->data(), ws.wins.data(), sizeof(WinDesc) * ws.wins.size());
  std::memcpy(blob->data() + l.off_lag, ws.lag.data(), sizeof(double) * ws.lag.size());
  std::memcpy(blob->data() + l.off_lagh, ws.lag_h.data(), sizeof(double) * ws.lag_h.size());
  std::memcpy(blob->data() + l.off_lagsd, ws.lag_sd.data(), sizeof(double) * ws.lag_sd.size());
}

void blank_rows(const uint8_t* valid, int64_t nrows, const RowArray* arrays, int narrays) {
  const double qnan = std::nan("");
  for (int64_t i = 0; i < nrows; ++i) {
    if (valid[i] != 2) continue;
    for (int k = 0; k < narrays; ++k) {
      if (!arrays[k].p) continue;
      double* row = arrays[k].p + (size_t)i * arrays[k].per;
      for (size_t o = 0; o < arrays[k].per; ++o) row[o] = qnan;
    }
  }
}

}  // namespace mwrt
