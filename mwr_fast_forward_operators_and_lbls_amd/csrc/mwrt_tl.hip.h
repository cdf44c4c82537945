// mwrt_tl.hip.h -- the device K-matrix path (csrc/mwrt_tl.hip): tangent-linear absorption + adjoint RTE.  Argument
// records and launchers only, as the host unit reads them; the device helpers the kernels use are included by mwrt_tl.hip.
//
// Two kernels, each in this one translation unit (built by build.py next to the chunk-width units):
//   k_absorb_tl  clearsky_absorption and its exact partial derivatives with respect to T (at fixed e) and e (at
//                fixed T) for every level and frequency: every line at every frequency, no far-line forms, no windows
//   k_jac_rte    the layer rule + Planck-space RTE + bright and their adjoint, fed by those six arrays;
//                with cloud liquid / ice it forms their absorption and its tangents itself; with retrieval
//                variables it changes the rows' variables before it stores them
#pragma once
#include "mwrt_args.hip.h"

namespace mwrt {

constexpr int TL_NFC = 7;          // frequencies per workgroup of k_absorb_tl (the HATPRO list: two chunks)

struct AbsorbTlArgs {
  const ModelFlat* M;
  const double* p; const double* t; const double* rh;         // [nprof][nlev]
  const double* frq;                                          // [nf], device copy
  double* awet; double* adry;                                 // [nprof][nf][nlev], Np/km
  double* dawet_dt; double* dawet_de; double* dadry_dt; double* dadry_de;   // Np/km/K, Np/km/hPa
  unsigned* flags;                                            // [nprof] or null: |= 1 NaN met, |= 2 negative absorption
  int nlev, nf, nslab;                                        // nslab = ceil(nlev / 64) one-wave level slabs per profile
};

struct JacRteArgs {
  const ModelFlat* M;
  const double* z; const double* t;                           // [nprof][nlev]
  const double* awet; const double* adry;                     // [nprof][nf][nlev] as k_absorb_tl writes them
  const double* dawet_dt; const double* dawet_de; const double* dadry_dt; const double* dadry_de;
  const unsigned* flags;                                      // [nprof] from k_absorb_tl
  const double* denliq; const double* denice;                 // [nprof][nlev] g m-3, either may be null (both: clear sky)
  const double* frq; const double* airmass;                   // [nf], [nang] device copies
  double* tb;                                                 // [nprof][nang][nf]
  double* dtb_dt; double* dtb_de; double* dtb_ddz;            // [nprof][nang][nf][nlev]
  double* dtb_dliq; double* dtb_dice;                         // the same layout, K per g m-3; null = not wanted
  uint8_t* valid;                                             // [nprof]
  int nlev, nf, nang;
  // retrieval variables (mwrt_jac_variables); all three 0: the rows above as they are.  dtb_ddz may then
  // be null (the raw thickness row is not wanted); dtb_de holds the humidity row, dtb_dliq / dtb_dice K per kg/kg
  const double* p; const double* rh;                          // [nprof][nlev], read only when a mode is set
  int humidity, cloud, heights;
};

constexpr int JAC_VARS_ROWS = 9;   // LDS rows of a launch with a retrieval-variable mode set, behind the cloud rows

hipError_t launch_absorb_tl(const AbsorbTlArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_jac_rte(const JacRteArgs& a, int64_t nprof, hipStream_t st);

}  // namespace mwrt
