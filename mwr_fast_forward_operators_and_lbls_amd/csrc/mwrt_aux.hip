// mwrt_aux.hip -- the kernels that are no templates, in a translation unit of their own, and their launchers: the
// ray-path pre-kernel of ray_tracing=True (k_ray_paths) and the self-tests of the arithmetic helpers (k_selftest_math;
// k_selftest_poly / _cplx / _planck / _layer / _layer4 / _div_small / _block / _votes behind mwrt_selftest_helpers).
// Declarations: mwrt_args.hip.h.  (The K-matrix kernels are csrc/mwrt_tl.hip.)
#include "mwrt_absorption.hip.h"
#include "mwrt_tl_dev.hip.h"          // hui_w_dw, layer_value_tl, the workgroup scans; mwrt_layer.hip.h through it

namespace mwrt {

// RTEquation.ray_tracing [EXT] (TBMODEL RAYTRAC: Dutton, Thayer & Westwater after Bean & Dutton fig. 3.20).
// Stores the PATH FACTOR ds_i / dz_i per layer, amf [nprof][nang][nlev] (entry 0 = 0): the slant-path
// integration multiplies the zenith layer optical depth by it, exactly where the plane-parallel path
// multiplies by 1/sin(elev).
//
// Workgroup = profile, LANE = LEVEL, loop over angles.  The reference walks the levels serially, carrying
// (phi, tau, r, tan theta) of the level below; but theta_i depends only on level i and the ground, and the
// carried sums enter ds only through differences,
//     phi_i - phi_{i-1} = (dtheta_i - dtheta_{i-1}) + dtau_i,      |tau_i - tau_{i-1}| = |dtau_i|,
// so every layer needs just its lower neighbour (one __shfl_up, wave seams through LDS): no scan, and the
// differences are formed directly instead of from two running sums (slightly better conditioned than the
// reference's own order; agreement ~1e-12 relative in ds).  A trapped ray (ducting: argth <= 0 at any level)
// gives NaN factors for that angle and duct[profile] = 1.  libm calls (asin, tan, ...): ~3 % of the opt-in
// path's arithmetic, not tuned further.
constexpr double EARTH_RADIUS_KM = 6370.949;
__global__ void __launch_bounds__(1024)
k_ray_paths(const double* __restrict__ z, const double* __restrict__ p, const double* __restrict__ t,
            const double* __restrict__ rh, int nlev, const double* __restrict__ elev_deg, int nang,
            double* __restrict__ amf, uint8_t* __restrict__ duct) {
  __shared__ double seam[16][3];            // last lane of each wave: refractive index, tan(theta), dtheta
  const int64_t prof = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const bool active = tid < nlev;
  const int64_t off = prof * nlev + (active ? tid : 0);
  const double qnan = __builtin_nan("");
  const double z0 = z[prof * nlev];
  const double zi = z[off] - z0;
  const double pi = p[off], ti = t[off], rhi = rh[off];
  const bool bad_prof = __syncthreads_or(active && (isnan(zi) || isnan(pi) || isnan(ti) || isnan(rhi)));
  const double ni = thayer_refindex(pi, ti, goff_gratch_e(ti, rhi));
  // neighbour level i-1 (level-only quantities)
  if (lane == WAVE - 1) seam[wave][0] = ni;
  __syncthreads();
  double nprev = __shfl_up(ni, 1, WAVE);
  double zprev = __shfl_up(zi, 1, WAVE);
  if (lane == 0 && wave > 0) { nprev = seam[wave - 1][0]; zprev = z[off - 1] - z0; }
  const double n0 = thayer_refindex(p[prof * nlev], t[prof * nlev], goff_gratch_e(t[prof * nlev], rh[prof * nlev]));
  const double rs = EARTH_RADIUS_KM + 0.0 + z0;
  const double r = EARTH_RADIUS_KM + zi + z0;
  const double rl = EARTH_RADIUS_KM + zprev + z0;
  const double dz = zi - zprev;
  double refbar;
  if (ni == nprev || ni == 1.0 || nprev == 1.0) refbar = (ni + nprev) * 0.5;
  else refbar = 1.0 + (nprev - ni) / (log((nprev - 1.0) / (ni - 1.0)));
  for (int a = 0; a < nang; ++a) {
    double* out = amf + (prof * nang + a) * nlev;
    const double angle = elev_deg[a];
    if (bad_prof || isnan(angle)) {            // NaN inputs are the main kernel's business
      if (active) out[tid] = tid == 0 ? 0.0 : qnan;
      continue;
    }
    if ((angle >= 89.0 && angle <= 91.0) || (angle >= -91.0 && angle <= -89.0)) {
      if (active) out[tid] = (tid > 0 && dz != 0.0) ? 1.0 : 0.0;
      continue;
    }
    const double theta0 = angle * (M_PI / 180.0);
    const double costh0 = cos(theta0), sina = sin(theta0 * 0.5);
    const double a0 = 2.0 * (sina * sina);
    // my level: theta_i, dtheta_i (level 0 is the ground: theta0, 0)
    const double argdth = zi / rs - ((n0 - ni) * costh0 / ni);
    const double argth = 0.5 * (a0 + argdth) / r;
    const bool trapped_here = active && tid > 0 && !(argth > 0.0);
    double theta = theta0, dtheta = 0.0;
    if (tid > 0 && argth > 0.0) {
      const double sint = sqrt(r * argth);
      theta = 2.0 * asin(sint);
      if ((theta - 2.0 * theta0) <= 0.0) {
        const double dendth = 2.0 * (sint + sina) * cos((theta + theta0) * 0.25);
        const double sind4 = (0.5 * argdth - zi * argth) / dendth;
        dtheta = 4.0 * asin(sind4);
        theta = theta0 + dtheta;
      } else {
        dtheta = theta - theta0;
      }
    }
    const double tanth = tan(theta);
    __syncthreads();                             // previous angle's seam reads are done
    if (lane == WAVE - 1) { seam[wave][1] = tanth; seam[wave][2] = dtheta; }
    const bool trapped = __syncthreads_or(trapped_here);
    double tanthl = __shfl_up(tanth, 1, WAVE);
    double dthl = __shfl_up(dtheta, 1, WAVE);
    if (lane == 0 && wave > 0) { tanthl = seam[wave - 1][1]; dthl = seam[wave - 1][2]; }
    double f = 0.0;
    if (tid > 0) {
      const double cthbar = ((1.0 / tanth) + (1.0 / tanthl)) * 0.5;
      const double dtau = cthbar * (nprev - ni) / refbar;
      const double dphi = (dtheta - dthl) + dtau;
      const double sh = sin(dphi * 0.5);
      double dsi = sqrt(dz * dz + 4.0 * r * rl * (sh * sh));
      if (dtau != 0.0) {
        const double dtaua = fabs(dtau);
        dsi = dsi * (dtaua / (2.0 * sin(dtaua * 0.5)));
      }
      f = (dz != 0.0) ? dsi / dz : 0.0;
    }
    if (active) out[tid] = trapped ? (tid == 0 ? 0.0 : qnan) : f;     // pyrtlib gives up on the whole ray
    if (trapped && tid == 0) duct[prof] = 1;
  }
}

// diagnostic: the local exp / log / division helpers on caller-supplied arguments (mwrt_selftest_math)
__global__ void k_selftest_math(const double* x, const double* y, double* out_exp, double* out_log, double* out_div,
                                double* out_div1, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out_exp[i] = fexp(x[i]);
  out_log[i] = flog(y[i]);
  out_div[i] = fdiv(x[i], y[i]);
  out_div1[i] = fdiv1(x[i], y[i]);
}

// diagnostic: the other helpers, each called as shipped on caller-supplied arguments (mwrt_selftest_helpers; the table of
// selectors is in include/mwrt.h).  One thread per element; a thread past n leaves BEFORE the helper is called, so the
// last wave takes every vote with inactive lanes.  Several kernels: the polynomial constants ride in SGPR pairs.
__global__ void __launch_bounds__(1024) k_selftest_poly(HelperArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const double x = a.in[0][i];
  switch (a.helper) {
    case MWRT_HELPER_FEXP_SMALL:
      a.out[0][i] = fexp_small(x);
      a.out[1][i] = fexp_small(x, loop_invariant_vgpr(FEXP_SMALL_C0));
      break;
    case MWRT_HELPER_FEXP_TINY: a.out[0][i] = fexp_tiny(x); break;
    case MWRT_HELPER_FTANH_HALF_SMALL:
      a.out[0][i] = ftanh_half_small(x);
      a.out[1][i] = ftanh_half_small(x, loop_invariant_vgpr(FTANH_HALF_SMALL_C0));
      break;
    case MWRT_HELPER_FTANH_HALF_TINY: a.out[0][i] = ftanh_half_tiny(x); break;
    case MWRT_HELPER_TWO_ATANH_TAIL: a.out[0][i] = two_atanh_tail(x); break;
    default: a.out[0][i] = fsqrt(x); break;
  }
}

__global__ void __launch_bounds__(1024) k_selftest_cplx(HelperArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const cplx z = {a.in[0][i], a.in[1][i]};
  cplx r = {0.0, 0.0}, r2 = {0.0, 0.0};
  switch (a.helper) {
    case MWRT_HELPER_CRECIP: r = crecip(z); break;
    case MWRT_HELPER_CMUL_CDIV: {
      const cplx b = {a.in[2][i], a.in[3][i]};
      r = cmul(z, b);
      r2 = cdiv(z, b);
      break;
    }
    case MWRT_HELPER_CSQRT_PRINCIPAL: r = csqrt_principal(z); break;
    case MWRT_HELPER_DCERROR_UPPER: r = dcerror_upper(z.re, z.im); break;
    default: hui_w_dw(z, r, r2); break;
  }
  a.out[0][i] = r.re; a.out[1][i] = r.im;
  a.out[2][i] = r2.re; a.out[3][i] = r2.im;
}

__global__ void __launch_bounds__(1024) k_selftest_planck(HelperArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  a.out[0][i] = planck_b(a.in[0][i], a.in[1][i]);
}

__global__ void __launch_bounds__(1024) k_selftest_layer(HelperArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const double x1 = a.in[0][i], x0 = a.in[1][i];
  const bool live = a.in[2][i] != 0.0;
  bool neg = false;
  double d1 = 0.0, d0 = 0.0, r;
  switch (a.helper) {
    case MWRT_HELPER_LAYER_VALUE_ZF1: r = layer_value<true>(x1, x0, neg, live); break;
    case MWRT_HELPER_LAYER_VALUE_ZF0: r = layer_value<false>(x1, x0, neg, live); break;
    case MWRT_HELPER_LAYER_VALUE_TL_ZF1: r = layer_value_tl<true>(x1, x0, d1, d0, neg); break;
    default: r = layer_value_tl<false>(x1, x0, d1, d0, neg); break;
  }
  a.out[0][i] = r; a.out[1][i] = d1; a.out[2][i] = d0;
  a.flag[i] = neg ? 1 : 0;
}

// one thread per four consecutive elements (n is a multiple of 4)
__global__ void __launch_bounds__(1024) k_selftest_layer4(HelperArgs a) {
  const int64_t i = 4 * (blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
  if (i >= a.n) return;
  double x1[4], x0[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { x1[k] = a.in[0][i + k]; x0[k] = a.in[1][i + k]; }
  bool neg = false;
  layer_value4(x1, x0, neg, a.in[2][i] != 0.0);
#pragma unroll
  for (int k = 0; k < 4; ++k) { a.out[0][i + k] = x1[k]; a.flag[i + k] = neg ? 1 : 0; }
}

__global__ void __launch_bounds__(1024) k_selftest_div_small(HelperArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  a.out[0][i] = (double)div_small((int)a.in[0][i], (int)a.in[1][i], (unsigned)a.in[2][i]);
}

// the collectives: one workgroup per blockDim.x elements, every thread in the call (those past n hold 0)
__global__ void __launch_bounds__(1024) k_selftest_block(HelperArgs a) {
  __shared__ double wsum[1024 / WAVE];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + tid;
  const bool inside = i < a.n;
  const double v = inside ? a.in[0][i] : 0.0;
  const int nwaves = (int)blockDim.x / WAVE;
  double r, total = 0.0;
  switch (a.helper) {
    case MWRT_HELPER_BLOCK_SUM: r = block_sum(v, wsum, tid, (int)blockDim.x); break;
    case MWRT_HELPER_BLOCK_SCAN: r = block_scan(v, wsum, tid, nwaves, total); break;
    case MWRT_HELPER_BLOCK_SUFFIX_EXCL: r = block_suffix_excl(v, wsum, tid, nwaves); break;
    default: r = (double)row16_max((float)v); break;
  }
  if (inside) { a.out[0][i] = r; a.out[1][i] = total; }
}

__global__ void __launch_bounds__(1024) k_selftest_votes(HelperArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const bool p = a.in[0][i] != 0.0, q = a.in[1][i] != 0.0;
  a.out[0][i] = wave_all(p) ? 1.0 : 0.0;
  a.out[1][i] = wave_any(p) ? 1.0 : 0.0;
  a.out[2][i] = wave_all_of(p, q) ? 1.0 : 0.0;
}

hipError_t launch_selftest_helpers(const HelperArgs& a, int block, hipStream_t st) {
  const int64_t threads = a.helper == MWRT_HELPER_LAYER_VALUE4 ? a.n / 4 : a.n;
  const dim3 grid((unsigned)((threads + block - 1) / block)), blk((unsigned)block);
  const int h = a.helper;
  if (h <= MWRT_HELPER_FSQRT) hipLaunchKernelGGL(k_selftest_poly, grid, blk, 0, st, a);
  else if (h <= MWRT_HELPER_HUI_W_DW) hipLaunchKernelGGL(k_selftest_cplx, grid, blk, 0, st, a);
  else if (h == MWRT_HELPER_PLANCK_B) hipLaunchKernelGGL(k_selftest_planck, grid, blk, 0, st, a);
  else if (h == MWRT_HELPER_LAYER_VALUE4) hipLaunchKernelGGL(k_selftest_layer4, grid, blk, 0, st, a);
  else if (h <= MWRT_HELPER_LAYER_VALUE_TL_ZF0) hipLaunchKernelGGL(k_selftest_layer, grid, blk, 0, st, a);
  else if (h == MWRT_HELPER_DIV_SMALL) hipLaunchKernelGGL(k_selftest_div_small, grid, blk, 0, st, a);
  else if (h <= MWRT_HELPER_ROW16_MAX) hipLaunchKernelGGL(k_selftest_block, grid, blk, 0, st, a);
  else hipLaunchKernelGGL(k_selftest_votes, grid, blk, 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ray_paths(const double* z,const double* p, const double* t, const double* rh, int64_t nprof, int nlev,
                            const double* elev_deg, int nang, double* amf, uint8_t* duct, hipStream_t st) {
  hipLaunchKernelGGL(k_ray_paths, dim3((unsigned)nprof), dim3(lanes_for(nlev)), 0, st, z, p, t, rh, nlev, elev_deg, nang, amf,
                     duct);
  return hipGetLastError();
}

hipError_t launch_selftest_math(const double* x, const double* y, double* out_exp, double* out_log, double* out_div,
                                double* out_div1, int n, hipStream_t st) {
  hipLaunchKernelGGL(k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, st, x, y, out_exp, out_log, out_div, out_div1, n);
  return hipGetLastError();
}

}  // namespace mwrt
