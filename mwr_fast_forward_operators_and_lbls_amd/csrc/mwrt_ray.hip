// mwrt_ray.hip -- the device K-matrix along refracted spherical ray paths: the path factors of ray_tracing = 1 with their
// exact partial derivatives (k_ray_paths_tl) and the adjoint RTE that consumes them (k_jac_rte_ray).  Declarations and
// argument records: mwrt_ray.hip.h; entry points: mwrt_tb_jacobian_batch_ray_device / mwrt_tb_jacobian_batch_ray in mwrt.hip;
// the mathematics: DESIGN.md section 4.5.4.
#include "mwrt_ray.hip.h"
#include "mwrt_tl_rte.hip.h"          // jac_rte_body: the adjoint RTE (shared with mwrt_tl.hip)

namespace mwrt {
namespace ray {

namespace {

// ---------------------------------------------------------------------------------------------
// Forward-mode tangents in N directions, for the few dozen statements of the ray tracer: the value of every operation is
// the value k_ray_paths forms (the same statement, the same order); the tangent is that statement's own derivative.
// ---------------------------------------------------------------------------------------------
template <int N> struct dual { double v; double d[N]; };

template <int N> __device__ __forceinline__ dual<N> constant(double v) {
  dual<N> r; r.v = v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = 0.0;
  return r;
}
template <int N> __device__ __forceinline__ dual<N> variable(double v, int slot) {
  dual<N> r = constant<N>(v);
#pragma unroll
  for (int k = 0; k < N; ++k) if (k == slot) r.d[k] = 1.0;
  return r;
}
// g(a) with g'(a.v) = slope
template <int N> __device__ __forceinline__ dual<N> chain(dual<N> a, double value, double slope) {
  dual<N> r; r.v = value;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * slope;
  return r;
}
template <int N> __device__ __forceinline__ dual<N> operator+(dual<N> a, dual<N> b) {
  dual<N> r; r.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
template <int N> __device__ __forceinline__ dual<N> operator-(dual<N> a, dual<N> b) {
  dual<N> r; r.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
template <int N> __device__ __forceinline__ dual<N> operator*(dual<N> a, dual<N> b) {
  dual<N> r; r.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
template <int N> __device__ __forceinline__ dual<N> operator/(dual<N> a, dual<N> b) {
  dual<N> r; r.v = a.v / b.v;
  const double ib = 1.0 / b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * ib;
  return r;
}
template <int N> __device__ __forceinline__ dual<N> operator+(dual<N> a, double s) { a.v = a.v + s; return a; }
template <int N> __device__ __forceinline__ dual<N> operator+(double s, dual<N> a) { a.v = s + a.v; return a; }
template <int N> __device__ __forceinline__ dual<N> operator-(dual<N> a, double s) { a.v = a.v - s; return a; }
template <int N> __device__ __forceinline__ dual<N> operator*(dual<N> a, double s) { return chain(a, a.v * s, s); }
template <int N> __device__ __forceinline__ dual<N> operator*(double s, dual<N> a) { return chain(a, s * a.v, s); }
template <int N> __device__ __forceinline__ dual<N> operator/(dual<N> a, double s) { return chain(a, a.v / s, 1.0 / s); }
template <int N> __device__ __forceinline__ dual<N> operator/(double s, dual<N> a) {
  const double q = s / a.v;
  return chain(a, q, -q / a.v);
}
template <int N> __device__ __forceinline__ dual<N> dsqrt(dual<N> a) { const double s = sqrt(a.v); return chain(a, s, 0.5 / s); }
template <int N> __device__ __forceinline__ dual<N> dasin(dual<N> a) { return chain(a, asin(a.v), 1.0 / sqrt(1.0 - a.v * a.v)); }
template <int N> __device__ __forceinline__ dual<N> dsin(dual<N> a) { return chain(a, sin(a.v), cos(a.v)); }
template <int N> __device__ __forceinline__ dual<N> dcos(dual<N> a) { return chain(a, cos(a.v), -sin(a.v)); }
template <int N> __device__ __forceinline__ dual<N> dtan(dual<N> a) { const double t = tan(a.v); return chain(a, t, 1.0 + t * t); }
template <int N> __device__ __forceinline__ dual<N> dlog(dual<N> a) { return chain(a, log(a.v), 1.0 / a.v); }
template <int N> __device__ __forceinline__ dual<N> dfabs(dual<N> a) { return chain(a, fabs(a.v), a.v < 0.0 ? -1.0 : 1.0); }

// ---------------------------------------------------------------------------------------------
// k_ray_paths_tl: k_ray_paths (mwrt_aux.hip: workgroup = profile, lane = level, loop over elevations) with tangents.
// theta_i and dtheta_i depend on level i and the ground only -- on (n_i, n_0, z_i), z the height above the ground level
// with z_0 itself held -- so they carry three tangents, and a layer needs its lower neighbour's: one __shfl_up each, the
// wave seams through LDS.  The layer's factor then depends on (n_l, n_{l-1}, n_0, z_l, z_{l-1}): five tangents, stored
// behind f as rows 1 - 5 of path [nprof][nang][6][nlev].  The branches are the forward's, in its order -- refbar's equal /
// unit-index branch, theta - 2 theta0 <= 0, dtau != 0 -- and the tangent is that of the branch taken.  Two deliberate
// differences, neither of which changes a TB: within 1 degree of zenith the factor is 1 for a zero-thickness layer too (the
// branch returns ds = dz, so its derivative towards the thickness is 1; the forward kernel writes 0 there, and the layer's
// optical depth is 0 either way); every other zero-thickness layer has f = 0 and no tangent, as in the forward kernel.
// A trapped ray gives NaN rows for its elevation and duct[profile] = 1; NaN inputs are the RTE kernel's business.
// ---------------------------------------------------------------------------------------------
constexpr double EARTH_RADIUS_KM = 6370.949;       // as k_ray_paths

__global__ void __launch_bounds__(1024)
k_ray_paths_tl(const PathTlArgs A) {
  typedef dual<3> D3;                        // slots: n_i, n_0, z_i
  typedef dual<5> D5;                        // slots: n_l, n_{l-1}, n_0, z_l, z_{l-1}
  __shared__ double seam[16][9];             // last lane of each wave: n, then tan(theta) and dtheta with three tangents each
  const int nlev = A.nlev, nang = A.nang;
  const int64_t prof = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const bool active = tid < nlev;
  const int64_t off = prof * nlev + (active ? tid : 0);
  const double qnan = __builtin_nan("");
  const double z0 = A.z[prof * nlev];
  const double zi = A.z[off] - z0;
  const double pi = A.p[off], ti = A.t[off], rhi = A.rh[off];
  const bool bad_prof = __syncthreads_or(active && (isnan(zi) || isnan(pi) || isnan(ti) || isnan(rhi)));
  const double ni = thayer_refindex(pi, ti, goff_gratch_e(ti, rhi));
  if (lane == WAVE - 1) seam[wave][0] = ni;
  __syncthreads();
  double nprev = __shfl_up(ni, 1, WAVE);
  double zprev = __shfl_up(zi, 1, WAVE);
  if (lane == 0 && wave > 0) { nprev = seam[wave - 1][0]; zprev = A.z[off - 1] - z0; }
  const double n0 = thayer_refindex(A.p[prof * nlev], A.t[prof * nlev], goff_gratch_e(A.t[prof * nlev], A.rh[prof * nlev]));
  const double rs = EARTH_RADIUS_KM + 0.0 + z0;
  const double r = EARTH_RADIUS_KM + zi + z0;
  const double rl = EARTH_RADIUS_KM + zprev + z0;
  const double dz = zi - zprev;
  const D5 nu = variable<5>(ni, 0), nl = variable<5>(nprev, 1);
  D5 refbar;
  if (ni == nprev || ni == 1.0 || nprev == 1.0) refbar = (nu + nl) * 0.5;
  else refbar = 1.0 + (nl - nu) / dlog((nl - 1.0) / (nu - 1.0));
  const D5 dn = nl - nu;
  D5 ru = constant<5>(r), rlo = constant<5>(rl);
  ru.d[3] = 1.0; rlo.d[4] = 1.0;
  const D5 dzd = variable<5>(zi, 3) - variable<5>(zprev, 4);
  const D5 rr4 = 4.0 * ru * rlo;
  for (int a = 0; a < nang; ++a) {
    double* out = A.path + (prof * nang + a) * ((int64_t)PATH_ROWS * nlev);
    auto store = [&](double f, double d0, double d1, double d2, double d3, double d4) {
      if (!active) return;
      out[tid] = f; out[nlev + tid] = d0; out[2 * nlev + tid] = d1; out[3 * nlev + tid] = d2; out[4 * nlev + tid] = d3;
      out[5 * nlev + tid] = d4;
    };
    const double angle = A.elev_deg[a];
    if (bad_prof || isnan(angle)) {
      const double v = tid == 0 ? 0.0 : qnan;
      store(v, v, v, v, v, v);
      continue;
    }
    if ((angle >= 89.0 && angle <= 91.0) || (angle >= -91.0 && angle <= -89.0)) {
      store(tid > 0 ? 1.0 : 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
      continue;
    }
    const double theta0 = angle * (M_PI / 180.0);
    const double costh0 = cos(theta0), sina = sin(theta0 * 0.5);
    const double a0 = 2.0 * (sina * sina);
    // my level: theta_i, dtheta_i (level 0 is the ground: theta0, 0)
    const D3 n3 = variable<3>(ni, 0), g3 = variable<3>(n0, 1), z3 = variable<3>(zi, 2);
    D3 r3 = constant<3>(r);
    r3.d[2] = 1.0;
    const D3 argdth = z3 / rs - ((g3 - n3) * costh0 / n3);
    const D3 argth = 0.5 * (a0 + argdth) / r3;
    const bool trapped_here = active && tid > 0 && !(argth.v > 0.0);
    D3 theta = constant<3>(theta0), dtheta = constant<3>(0.0);
    if (tid > 0 && argth.v > 0.0) {
      const D3 sint = dsqrt(r3 * argth);
      theta = 2.0 * dasin(sint);
      if ((theta.v - 2.0 * theta0) <= 0.0) {
        const D3 dendth = 2.0 * (sint + sina) * dcos((theta + theta0) * 0.25);
        const D3 sind4 = (0.5 * argdth - z3 * argth) / dendth;
        dtheta = 4.0 * dasin(sind4);
        theta = theta0 + dtheta;
      } else {
        dtheta = theta - theta0;
      }
    }
    const D3 tanth = dtan(theta);
    __syncthreads();                             // previous elevation's seam reads are done
    if (lane == WAVE - 1) {
      seam[wave][1] = tanth.v; seam[wave][5] = dtheta.v;
#pragma unroll
      for (int k = 0; k < 3; ++k) { seam[wave][2 + k] = tanth.d[k]; seam[wave][6 + k] = dtheta.d[k]; }
    }
    const bool trapped = __syncthreads_or(trapped_here);
    D3 tanthl, dthl;
    tanthl.v = __shfl_up(tanth.v, 1, WAVE); dthl.v = __shfl_up(dtheta.v, 1, WAVE);
#pragma unroll
    for (int k = 0; k < 3; ++k) { tanthl.d[k] = __shfl_up(tanth.d[k], 1, WAVE); dthl.d[k] = __shfl_up(dtheta.d[k], 1, WAVE); }
    if (lane == 0 && wave > 0) {
      tanthl.v = seam[wave - 1][1]; dthl.v = seam[wave - 1][5];
#pragma unroll
      for (int k = 0; k < 3; ++k) { tanthl.d[k] = seam[wave - 1][2 + k]; dthl.d[k] = seam[wave - 1][6 + k]; }
    }
    if (trapped) {                               // pyrtlib gives up on the whole ray
      const double v = tid == 0 ? 0.0 : qnan;
      store(v, v, v, v, v, v);
      if (tid == 0) A.duct[prof] = 1;
      continue;
    }
    D5 f = constant<5>(0.0);
    if (tid > 0 && dz != 0.0) {
      // the level's three directions among the layer's five: the upper end is (n_l, n_0, z_l), the lower (n_{l-1}, n_0, z_{l-1})
      D5 tu = constant<5>(tanth.v), du = constant<5>(dtheta.v), tl = constant<5>(tanthl.v), dl = constant<5>(dthl.v);
      tu.d[0] = tanth.d[0]; tu.d[2] = tanth.d[1]; tu.d[3] = tanth.d[2];
      du.d[0] = dtheta.d[0]; du.d[2] = dtheta.d[1]; du.d[3] = dtheta.d[2];
      tl.d[1] = tanthl.d[0]; tl.d[2] = tanthl.d[1]; tl.d[4] = tanthl.d[2];
      dl.d[1] = dthl.d[0]; dl.d[2] = dthl.d[1]; dl.d[4] = dthl.d[2];
      const D5 cthbar = ((1.0 / tu) + (1.0 / tl)) * 0.5;
      const D5 dtau = cthbar * dn / refbar;
      const D5 dphi = (du - dl) + dtau;
      const D5 sh = dsin(dphi * 0.5);
      D5 dsi = dsqrt(dzd * dzd + rr4 * (sh * sh));
      if (dtau.v != 0.0) {
        const D5 dtaua = dfabs(dtau);
        dsi = dsi * (dtaua / (2.0 * dsin(dtaua * 0.5)));
      }
      f = dsi / dzd;
    }
    store(f.v, f.d[0], f.d[1], f.d[2], f.d[3], f.d[4]);
  }
}

__global__ void __launch_bounds__(1024)
k_jac_rte_ray(const RayRteArgs A) {
  jac_rte_body<true>(A.J, A.path, A.duct);
}

}  // namespace

hipError_t launch_ray_paths_tl(const PathTlArgs& a, int64_t nprof, hipStream_t st) {
  hipLaunchKernelGGL(k_ray_paths_tl, dim3((unsigned)nprof), dim3(lanes_for(a.nlev)), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_jac_rte_ray(const RayRteArgs& a, int64_t nprof, hipStream_t st) {
  const int threads = lanes_for(a.J.nlev);
  const size_t lds = jac_rte_lds_bytes(a.J, threads, true);
  if (lds > 64 * 1024) {                 // beyond the default dynamic LDS limit, as launch_jac_rte
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_jac_rte_ray),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_jac_rte_ray, dim3((unsigned)(nprof * a.J.nf)), dim3(threads), lds, st, a);
  return hipGetLastError();
}

}  // namespace ray
}  // namespace mwrt
