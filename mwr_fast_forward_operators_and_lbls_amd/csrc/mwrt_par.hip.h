// mwrt_par.hip.h -- the spectroscopic-parameter Jacobian (csrc/mwrt_par.hip; include/mwrt.h
// mwrt_tb_param_jacobian_batch_device).  Argument records and launchers only, as the host unit reads them.
//
// Two kernels behind k_absorb_tl (whose awet, adry and flags they read from the K-matrix workspace), launched once per
// GROUP of parameters -- as many as fit the tangent workspace, see PAR_WS_BYTES:
//   k_par_tangent   d alpha_l / d b for every (profile, frequency, parameter of the group, level): one wave = 64 levels
//                   of one profile at one frequency; one line's term for a per-line parameter, a sum over the species'
//                   lines for MWRT_PAR_O2_X and MWRT_PAR_ALL_LINES.  Written level-fastest (coalesced).
//   k_par_contract  one workgroup per (profile, frequency), one lane per level: k_jac_rte's clear-sky adjoint gives the
//                   level sensitivities d TB / d alpha_l per elevation; every parameter row is summed against them over the
//                   levels in a fixed order and stored parameter-fastest.
// Workspace: 8 B per (profile, frequency, level) and parameter of a group, owned by the context and only grown behind a
// drain, next to the 48 B per (profile, frequency, level) of the K-matrix workspace.
#pragma once
#include "mwrt_args.hip.h"

namespace mwrt {
namespace par {

// the tangent workspace is bounded by taking the parameters in groups: as many as fit this many bytes, at least one (a
// column's arithmetic does not depend on its group)
constexpr size_t PAR_WS_BYTES = (size_t)1 << 30;     // 1 GiB: 53 parameters at 1000 profiles x 14 channels x 180 levels
constexpr int CONTRACT_PB = 8;                    // parameters whose partial sums share one barrier in k_par_contract
constexpr int CONTRACT_SENS_BYTES = 16 * 1024;    // LDS for the sensitivities of a chunk of elevations: 5 at 180 levels, 1 at 1024

struct ParTangentArgs {
  const ModelFlat* M;
  const double* p; const double* t; const double* rh;         // [nprof][nlev]
  const double* frq;                                          // [nf], device copy
  const mwrt_param* params;                                   // [npar] device copy, validated by the host
  double* dalpha;                                             // [nprof][nf][gn][nlev], Np/km per unit of the entry
  int nlev, nf, nslab;                                        // nslab = ceil(nlev / 64) one-wave level slabs per profile
  int p0, gn;                                                 // the group: parameters p0 .. p0 + gn - 1
  int o2_any;                                                 // an O2 parameter is in the group: the max(o2abs, 0) clamp is looked for
};

struct ParContractArgs {
  const ModelFlat* M;
  const double* z; const double* t;                           // [nprof][nlev]
  const double* awet; const double* adry;                     // [nprof][nf][nlev] as k_absorb_tl writes them
  const unsigned* flags;                                      // [nprof] from k_absorb_tl
  const double* frq; const double* airmass;                   // [nf], [nang] device copies
  const mwrt_param* params;                                   // [npar] device copy
  const double* dalpha;                                       // [nprof][nf][gn][nlev] from k_par_tangent
  double* tb;                                                 // [nprof][nang][nf] or null; written with the first group
  double* dtb_db;                                             // [nprof][nang][nf][npar]
  uint8_t* valid;                                             // [nprof]; written with the first group
  int nlev, nf, nang, npar;
  int p0, gn;
  int achunk;                                                 // elevations per chunk (set by the launcher)
};

hipError_t launch_par_tangent(const ParTangentArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_par_contract(ParContractArgs a, int64_t nprof, hipStream_t st);

}  // namespace par
}  // namespace mwrt
