// mwrt_plan.h -- what host and device agree on (plain records and constants), and the host's launch planning:
// which kernel instantiation serves a call, how its work is split, and the tables it reads (csrc/mwrt_plan.cpp).
//
// Plain C++17 with no HIP in it: any host compiler builds the planning unit, so it can be run and sanitised without a
// GPU library (tests/plan_dump.cpp).  mwrt_args.hip.h includes this header; the device code is in the mwrt_*.hip.h headers behind it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/mwrt.h"

namespace mwrt {

constexpr int WAVE = 64;

struct LaunchGeom {          // host-computed K2 work split (see plan_k2 in mwrt_plan.cpp), per K2 pass
  int nseg[2];               // level segments per (freq, angle) pair
  int seglen[2];             // layers per segment
  int npart;                 // doubles of segment partials (B, T) the largest pass needs
  int ldrow;                 // padded LDS row length (doubles) of tau/boft: conflict-free for b64, > nseg * seglen of a sorted pass
  unsigned magic_nseg[2];    // ceil(2^32 / nseg), ceil(2^32 / nang): n / d = umulhi(n, magic) for n < 65536, 1 < d <= 1024
  unsigned magic_nang;       // (the work-item index splits cost two integer divisions per item otherwise)
};

// "Far" lines: every frequency of the chunk is at least FAR_MIN_GHZ (+ the shift allowance) away
// from the line centre, so D1*D2 may be formed as a polynomial in f^2 without harmful cancellation.
constexpr double FAR_MIN_GHZ = 0.2;
constexpr double FAR_SHIFT_GHZ = 0.05;     // O2: |dnu| allowance, checked per line by wave vote
constexpr double FAR_H2O_GHZ = 5.0;        // H2O: covers any pressure shift (< 1 GHz) with margin

// Wave-uniform bit sets over line indices (line k of the table against the chunk's frequencies).  They steer the line
// loops: each loop walks ONE set with ONE loop body, so the NFC accumulators never cross a
// control-flow join between differently allocated variants (the v_mov copies that cost).
struct LineMasks {
  unsigned long long o2_far;   // every chunk frequency >= FAR_MIN_GHZ + FAR_SHIFT_GHZ from the line centre
  unsigned h2o_far;            // ... >= FAR_H2O_GHZ from the line centre
  unsigned h2o_none;           // both Lorentz terms beyond the 750-GHz cutoff for every frequency (FAR_H2O_GHZ margin)
  unsigned h2o_res;            // negative-frequency term beyond the cutoff for every frequency (e.g. 752 GHz from 22 GHz)
  unsigned h2o_sd;             // speed-dependent lines (W2 > 0)
  unsigned h2o_sdfar;          // ... of those, the ones whose special shape (inside 10 half-widths) cannot reach any frequency of
                               // the chunk by the host's bound: treated as plain lines, re-checked per level (wave vote)
  unsigned h2o_sdint;          // speed-dependent lines far enough from the chunk (>= 3 GHz and 5 spans) for the half-sampled shape (SD_LEBESGUE_MAX)
  unsigned h2o_vfar;           // "very far" lines: summed as ONE Taylor polynomial in f^2 about the chunk's middle (vfar_add)
  unsigned long long o2_vfar;
  double vf_u0, vf_h, vf_invh; // middle and half range of the chunk's f^2 values [GHz^2] (vf_h >= 1), 1 / vf_h
};

// The sets the far-line loops of dry_absorb / h2o_absorb walk (mwrt_absorption.hip.h), shared by the kernels and by whoever
// wants to know what they run (tests/far_set_dump.cpp).  `n` = lines in the table.  *_far_set: loop A, the rational form --
// for water neither resonant-only, speed-dependent within reach nor beyond the cutoff.  *_vfar_set: of those (`far`), the
// very far lines, summed as one Taylor polynomial (`nodes`: the window's node phase has none).  *_quad_set: the rest; they go
// four at a time, the count mod 4 left over joins the general loop.
constexpr unsigned long long o2_lines_all(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
constexpr unsigned h2o_lines_all(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }
constexpr unsigned long long o2_far_set(const LineMasks& lm, unsigned long long all) { return lm.o2_far & all; }
constexpr unsigned long long o2_vfar_set(const LineMasks& lm, unsigned long long far, bool nodes) { return nodes ? 0ull : (far & lm.o2_vfar); }
constexpr unsigned long long o2_quad_set(const LineMasks& lm, unsigned long long far, bool nodes) { return far & ~o2_vfar_set(lm, far, nodes); }
constexpr unsigned h2o_sd_near(const LineMasks& lm) { return lm.h2o_sd & ~lm.h2o_sdfar; }   // straight to the speed-dependent loop
constexpr unsigned h2o_far_set(const LineMasks& lm, unsigned all) {
  return lm.h2o_far & ~lm.h2o_res & ~h2o_sd_near(lm) & ~lm.h2o_none & all;
}
constexpr unsigned h2o_vfar_set(const LineMasks& lm, unsigned far, bool nodes) { return nodes ? 0u : (far & lm.h2o_vfar); }
constexpr unsigned h2o_quad_set(const LineMasks& lm, unsigned far, bool nodes) { return far & ~h2o_vfar_set(lm, far, nodes); }

// very far lines (mwrt_absorption.hip.h vfar_add): the host picks them (chunk_masks) with the shift / width allowances
constexpr double VF_RATIO_MAX = 0.016;
constexpr int VF_MIN_FREQS = 7;              // ... and chunks with fewer frequencies than this are served directly
constexpr int VF_MIN_LINES = 4;              // fewer lines than this do not pay for the Horner pass (8 per frequency)

// half-sampled speed-dependent shape (mwrt_absorption.hip.h): evaluated at 9 of a chunk's 16 frequencies, interpolated to 7
constexpr int SD_NODES = 9, SD_TARGETS = 7;
constexpr int sd_node_slot(int n) { return n < 8 ? 2 * n : 15; }
// ... where the chunk's own slots interpolate stably: the sum of a target's |weights| (10.3 on an evenly spaced chunk)
// multiplies every rounding error of the nine sampled values, and 9 weights rounded to doubles still sum to 1 within
// 9 x 100 x 2^-53 = 1e-13.  Near-coincident frequencies next to a gap reach 1e4 and more: such a chunk is sampled in full.
constexpr double SD_LEBESGUE_MAX = 100.0;

constexpr int MAX_MULTI = 8;   // absorption models evaluated by one launch (the wrapper runs four)

// rows kept in LDS per K2 pass; a 14-wide chunk runs as passes of 8 and 6 rows, each with its own split
constexpr int NFK = 8;
// a pass whose segments are at least this long deals its work items to the lanes thin ones first (k_tb_fused); shorter
// segments: dealing the items out costs more than the thin step saves
constexpr int K2_SORT_MIN_SEGLEN = 16;

constexpr int TAU_NFC = 16;                   // tau rows are written in 16-frequency (128-byte) pieces
constexpr int tau_threads(int nlev) { return ((nlev - 1 + (WAVE - 2)) / (WAVE - 1)) * WAVE; }
// one lane per level, in whole waves: the workgroup of every other kernel
constexpr int lanes_for(int nlev) { return ((nlev + WAVE - 1) / WAVE) * WAVE; }

constexpr int WIN_NODES = 16;          // O2: lines from WIN_MARGIN_GHZ beyond the window
constexpr int WIN_NODES_H = 8;         // H2O: lines from WIN_H2O_MARGIN_GHZ beyond it -- so smooth across the window that 8
                                       // nodes do (convergence ~ 25^-n); a third less LDS = a fourth workgroup per CU
constexpr int WIN_CHUNKS = 8;          // chunks of a base window
constexpr int WIN_CHUNKS_MAX = 16;     // ... of a merged one (two neighbours with no line near either: one node phase for both)
constexpr int WIN_NFC = 16;

struct WinDesc {                       // one per window, built by the host (csrc/mwrt_plan.cpp: build_windows)
  double fnode[WIN_NODES];             // Chebyshev nodes of [f_lo, f_hi], GHz
  double fnode_h[WIN_NODES_H];
  double flo, fhi;                     // the window itself
  unsigned long long o2_far;           // O2 lines >= WIN_MARGIN_GHZ beyond the window
  unsigned h2o_far_both, h2o_far_res;  // H2O lines >= WIN_H2O_MARGIN_GHZ beyond the window with a cutoff state uniform across it
  int first_chunk, nchunks;            // chunks [first_chunk, first_chunk + nchunks) of the frequency list
  int pad0, pad1;
};

constexpr int RTE_THREADS = 256;

// ---- fine-grid absorption: windows of WIN_CHUNKS chunks, Chebyshev nodes, Lagrange matrices ----
constexpr double WIN_MARGIN_GHZ = 4.0;       // an O2 line is window-far when its centre is this far beyond the window (16 nodes)
constexpr double WIN_H2O_MARGIN_GHZ = 30.0;  // an H2O line: this far (8 nodes; the H2O table is sparse, few lines come closer)
constexpr double WIN_MAX_SPAN_GHZ = 6.0;     // widest window the 16-node interpolation is used on
constexpr double WIN_CUTOFF_GUARD_GHZ = 5.0; // the H2O 750-GHz cutoff must be this clearly in or out (pressure shifts < 1 GHz)

// ---------------------------------------------------------------------------------------------
// host planning (csrc/mwrt_plan.cpp)
// ---------------------------------------------------------------------------------------------
unsigned magic_of(int d);

// K2 split for a chunk width, shrunk until the workgroup's LDS fits `lds_max`; false if it cannot.  threads = 0: lanes_for(nlev)
bool plan_fused(int lds_max, int nfc, int nlev, int nf, int nang, LaunchGeom* g, size_t* lds, int threads = 0);
int pick_nfc(int nf);
int pick_nfc_fused(int chunk_width, int lds_max, int nlev, int nf, int nang);

bool any_nan(const double* x, int n);
bool all_nan(const double* x, int n);
// plane-parallel air mass 1 / sin(elev) per elevation; false if an elevation lies outside (0, 180) degrees
bool airmass_of(const double* elev, int nang, std::vector<double>* am);
// elevations of the next k_rte_tau launch when `rem` are left: up to 8, 10 whole, 9 as 5 + 4
int rte_tau_angles(int rem);
int tau_pitch_of(int nf);

// bytes of LDS a windowed absorption workgroup of `threads` lanes needs (dynamic node sums + static tables)
size_t absorb_win_lds_bytes(int threads);
bool windows_eligible(const double* frq, int nf);
// which absorption kernel serves a frequency list at `threads` lanes under mwrt_set_absorption_mode's `mode`
enum class AbsorbRoute { every_line, windowed, refused /* mode 2 and the windows cannot serve the call */ };
AbsorbRoute absorption_route(int mode, int lds_max, const double* frq, int nf, int threads);

// line_masks of every chunk of `nfc` frequencies (what the kernels' line loops are steered by)
void chunk_masks(const mwrt_model_desc& t, const double* frq, int nf, int nfc, std::vector<LineMasks>* out);

struct WindowSet {
  std::vector<WinDesc> wins;
  std::vector<double> lag, lag_h;       // [nwin][WIN_CHUNKS_MAX][nodes][WIN_NFC]
  std::vector<double> lag_sd;           // [nchunks][SD_TARGETS][SD_NODES]: odd slots of a chunk from slots 0, 2, ..., 14, 15
};
void build_windows(const mwrt_model_desc& t, const double* frq, int nf, WindowSet* ws);

// The device image of a WindowSet: descriptors | lag | lag_h | lag_sd, each part starting on a 256-byte boundary.
// The offsets follow from the window count and the frequency count alone.
struct WindowLayout { size_t off_lag, off_lagh, off_lagsd, total; };
WindowLayout window_layout(int nwin, int nf);
void pack_windows(const WindowSet& ws, int nf, std::vector<char>* blob);

// NaN into rows of host output arrays: row i of every array (`per` doubles each) where valid[i] == 2
struct RowArray { double* p; size_t per; };
void blank_rows(const uint8_t* valid, int64_t nrows, const RowArray* arrays, int narrays);

}  // namespace mwrt
