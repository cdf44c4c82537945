// mwrt_ray.hip.h -- the device K-matrix along refracted spherical ray paths (csrc/mwrt_ray.hip).  Argument
// records and launchers only, as the host unit reads them.
//
// Two kernels in namespace mwrt::ray, behind mwrt_tb_jacobian_batch_ray_device (k_absorb_tl of mwrt_tl.hip runs between them):
//   k_ray_paths_tl  k_ray_paths (mwrt_aux.hip) with tangents: the path factor f = ds / dz of every (profile, elevation, layer)
//                   and its five partial derivatives -- towards the refractive index of the layer's upper end, of its lower
//                   end and of the ground, and towards the relative heights of its two ends
//   k_jac_rte_ray   the adjoint RTE of mwrt_tl_rte.hip.h with a path factor per lane and the rows' path terms
#pragma once
#include "mwrt_tl.hip.h"

namespace mwrt {
namespace ray {

constexpr int PATH_ROWS = 6;       // f, df/dn_l, df/dn_{l-1}, df/dn_0, df/dz_l, df/dz_{l-1}

struct PathTlArgs {
  const double* z; const double* p; const double* t; const double* rh;   // [nprof][nlev]
  const double* elev_deg;                                                // [nang], device copy
  double* path;                                                          // [nprof][nang][PATH_ROWS][nlev]
  uint8_t* duct;                                                         // [nprof], preset to 0: |= 1 a ray was trapped
  int nlev, nang;
};

struct RayRteArgs {
  JacRteArgs J;                    // (airmass is not read)
  const double* path;              // as k_ray_paths_tl wrote it
  const uint8_t* duct;
};

hipError_t launch_ray_paths_tl(const PathTlArgs& a, int64_t nprof, hipStream_t st);
hipError_t launch_jac_rte_ray(const RayRteArgs& a, int64_t nprof, hipStream_t st);

}  // namespace ray
}  // namespace mwrt
