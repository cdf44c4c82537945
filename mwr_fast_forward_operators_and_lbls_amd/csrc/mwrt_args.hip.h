// mwrt_args.hip.h -- what the host unit (csrc/mwrt.hip) and the kernel units agree on: the device image of the tables,
// the argument record of every kernel and the launchers that take them.  Plain records and declarations only: no device
// code lives here, so the host unit compiles without parsing a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mwrt.h"
#include "mwrt_plan.h"      // the plain records and constants shared with the host's planning unit

// The one build switch that changes a record's layout (FusedArgs::phase) has its default here, where the host unit and
// the kernel units both see it; the switches that only change code: mwrt_math.hip.h.
// diagnostic build (tools/phase_timeline.sh): lane 0 of every wave of k_tb_fused stamps the 100-MHz wall clock at its phase
// boundaries into FusedArgs::phase [workgroup][wave][10] (slots 8, 9: HW_ID and XCC_ID of the wave).  Always 0 in the shipped library.
#ifndef MWRT_PHASE_CLOCK
#define MWRT_PHASE_CLOCK 0
#endif

namespace mwrt {

constexpr double TAUMAX = 125.0;
constexpr double TRANS_MIN = 5.1664206328378610e-55;   // exp(-TAUMAX)

// Device image of the tables: the ABI record plus host-precomputed reciprocals.  It is read
// through a CONSTANT-address-space pointer: the tables never change while a kernel runs, and
// that is what lets the compiler fetch them with s_load (scalar cache, SGPR operands) instead of
// 64 identical vector loads per wave.
// Per-line records (array of structs): what the fused kernel's line loops read for line k sits in
// one contiguous 128-byte record, so the compiler fetches it with one or two wide s_load and a
// single wait per iteration instead of a dozen dwordx2 loads in three dependent groups.
struct O2Rec { double f, s300rf2, be, w300, y0, y1, g0, g1, dnu0, dnu1, pad[6]; };      // 128 B
struct H2ORec { double fl, s1, b2, w0, x, w0s, xs, sh, xh, shs, xhs, aair, aself, w2, pad[2]; };   // 128 B
struct ModelFlat : mwrt_model_desc {
  double o2_rf2[MWRT_MAX_O2_LINES];      // 1 / F_k^2
  O2Rec o2r[MWRT_MAX_O2_LINES];
  H2ORec h2or[MWRT_MAX_H2O_LINES];
};
typedef const __attribute__((address_space(4))) ModelFlat* cmodel;
typedef const __attribute__((address_space(4))) double* cdoubles;

// k_tb_fused (csrc/mwrt_fused.hip.h)
struct FusedArgs {
  // blockIdx.x enumerates (model, profile): outputs are [nmodels][nprof]..., inputs [nprof]...
  const ModelFlat* Ms[MAX_MULTI];
  int64_t nprof_in;        // profiles per model
  const double* z; const double* p; const double* t; const double* rh;   // [nprof][nlev]
  const double* frq;       // [nf] device
  const double* airmass;   // [nang] device: 1/sin(elev)
  double* tb;              // [nprof][nang][nf]
  uint8_t* valid;          // [nprof]
  double* tbatm; double* tmr; double* tauwet; double* taudry;   // optional [nprof][nang][nf]
  double* taulay;          // optional [nprof][nf][nlev]
  int nlev, nf, nang;
  int write_valid;         // 1: this launch has one workgroup per profile and sets valid = 1 itself
  LaunchGeom g;
  // by-products and opt-in physics (read by the OPT / EXTRAS instantiations only; null / 0 otherwise)
  const double* denliq; const double* denice;   // [nprof][nlev] g m-3, either may be null
  const double* amf;       // [nprof][nang][nlev] ray-traced path factor ds/dz, or null (plane-parallel)
  const uint8_t* duct;     // [nprof] 1: a ray of this profile was trapped (valid = 3)
  double* tauliq; double* tauice;               // optional [nprof][nang][nf]
  // ALPHA instantiation (RTE from materialised absorption): awet, adry [nprof][nf][nlev] as k_absorb writes them
  const double* awet_in; const double* adry_in;
  const LineMasks* masks[MAX_MULTI];   // per model: LineMasks of every frequency chunk (host-computed)
  const double* o3n;       // OPT: ozone number density [nprof][nlev] molecules m-3, or null
#if MWRT_PHASE_CLOCK
  long long* phase;        // diagnostic build only: [nprof][4][10] wall-clock stamps + HW_ID, XCC_ID
#endif
};

// where the TAU absorption kernels write (csrc/mwrt_tau.hip.h)
struct TauOut {
  const double* z;         // [nprof][nlev] km (layer thickness)
  double* tau;             // [nprof][nlev][fpitch]; row 0 (the ground level) is 0
  uint8_t* valid;          // [nprof], preset to 1 by the host; lowered to 0 (NaN input) / raised to 2 (negative absorption)
  int fpitch;              // doubles between consecutive levels: a multiple of 16, >= 16 * ceil(nf / 16)
};

// k_absorb
struct AbsorbArgs {
  const ModelFlat* M;
  const double* p; const double* t; const double* rh;
  const double* frq;
  double* awet; double* adry;
  int nlev, nf;
  TauOut T;                // TAU instantiations only
  const LineMasks* masks;  // [nchunks]
};

// k_absorb_win
struct AbsorbWinArgs {
  const ModelFlat* M;
  const double* p; const double* t; const double* rh;
  const double* frq;
  const WinDesc* win;                  // [nwin]
  const double* lagrange;              // [nwin][WIN_CHUNKS_MAX][WIN_NODES][WIN_NFC]: weight of node m for target j of chunk c
  const double* lagrange_h;            // [nwin][WIN_CHUNKS_MAX][WIN_NODES_H][WIN_NFC]
  const LineMasks* masks;              // [nchunks of the list]: line_masks() of every chunk, precomputed (it depends on the
                                       // frequencies and the table only)
  const double* lag_sd;                // [nchunks][SD_TARGETS][SD_NODES]: the half-sampled SD shape's weights per chunk
  double* awet; double* adry;
  int nlev, nf;
  TauOut T;                            // TAU instantiations only
};

// k_rte_tau
struct RteTauArgs {
  const ModelFlat* M;
  const double* tau;       // [nprof][nlev][fpitch]
  const double* t;         // [nprof][nlev] K
  const double* frq;       // [nf] GHz
  const double* airmass;   // [nang]; elevations a0 .. a0 + NA - 1 are this launch's
  double* tb;              // [nprof][nang][nf]
  const uint8_t* valid;    // [nprof] as the absorption kernel left it: != 1 -> NaN rows
  int nlev, nf, nang, fpitch, a0;
};

// ---------------------------------------------------------------------------------------------
// launchers: each returns hipGetLastError() of its launch
// ---------------------------------------------------------------------------------------------
// The fused kernel exists in 3 frequency-chunk widths x 3 workgroup sizes x 3 feature sets; compiled in one
// translation unit that is ~2 minutes of hipcc.  Each chunk width is its own translation unit
// (csrc/mwrt_inst.hip with -DMWRT_INST_NFC=8|14|16), built in parallel by build.py and linked into libmwrt.so.

// feature set of a fused-kernel instantiation
enum FusedVariant {
  FUSED_TB_ONLY = 0,   // clear sky, plane-parallel, TB only: the throughput path (bench, the wrapper's batched call)
  FUSED_OPT = 1,       // + cloud liquid / ice and ray-traced paths (mwrt_tb_options), TB only
  FUSED_FULL = 2,      // + the other DataFrame columns and layer optical depths (mwrt_tb_extras)
  FUSED_FROM_ALPHA = 3 // layer integration + RTE from absorption coefficients already in HBM (no K1), TB only
};

#define MWRT_DECLARE_INST(N)                                                                                         \
  hipError_t launch_fused_nfc##N(const FusedArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t st, int variant); \
  hipError_t launch_absorb_nfc##N(const AbsorbArgs& a, dim3 grid, dim3 block, hipStream_t st);
MWRT_DECLARE_INST(8)
MWRT_DECLARE_INST(14)
MWRT_DECLARE_INST(16)
#undef MWRT_DECLARE_INST
// the windowed fine-grid absorption kernel exists for the 16-wide chunks only (csrc/mwrt_inst.hip, NFC = 16 unit)
hipError_t launch_absorb_win(const AbsorbWinArgs& a, dim3 grid, dim3 block, hipStream_t st, bool tau);
// ... and so do the layer-optical-depth form of the every-line absorption kernel and the RTE kernel that reads it
hipError_t launch_absorb_tau(const AbsorbArgs& a, dim3 grid, dim3 block, hipStream_t st);
hipError_t launch_rte_tau(const RteTauArgs& a, dim3 grid, size_t lds, hipStream_t st, int na);

// the non-template kernels (csrc/mwrt_aux.hip): one workgroup per profile and one lane per level; one thread per element
hipError_t launch_ray_paths(const double* z, const double* p, const double* t, const double* rh, int64_t nprof, int nlev,
                            const double* elev_deg, int nang, double* amf, uint8_t* duct, hipStream_t st);
hipError_t launch_selftest_math(const double* x, const double* y, double* out_exp, double* out_log, double* out_div,
                                double* out_div1, int n, hipStream_t st);
// mwrt_selftest_helpers: helper = MWRT_HELPER_*, in / out = four device arrays of n doubles each, flag[n]
struct HelperArgs {
  const double* in[4];
  double* out[4];
  uint8_t* flag;
  int n, helper;
};
hipError_t launch_selftest_helpers(const HelperArgs& a, int block, hipStream_t st);

}  // namespace mwrt
