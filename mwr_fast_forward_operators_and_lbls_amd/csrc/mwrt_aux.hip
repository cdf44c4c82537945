// mwrt_aux.hip -- the kernels that are no templates, in a translation unit of their own, and their launchers: the
// ray-path pre-kernel of ray_tracing=True (k_ray_paths), the finite-difference K-matrix (k_tb_jacobian) and the
// self-test of the arithmetic helpers (k_selftest_math).  Argument records and declarations: mwrt_args.hip.h.
#include "mwrt_absorption.hip.h"
#include "mwrt_layer.hip.h"

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

// ---------------------------------------------------------------------------------------------
// K-matrix: dTB/dT, dTB/de, dTB/d(layer thickness) per level from ONE pass -- the adjoint of the layer rule and of
// the Planck-space recursion (RTEquation.exponential_integration / planck / bright [EXT]) applied to absorption
// derivatives.  The reference parses exactly this block out of RTTOV-gb's K run (RTTOV_gb_processing.py:286-300,
// :418-432); round 2 produced it with 3 nlev + 1 forward runs.
//
// Inputs: absorption at the profile's levels and at four locally perturbed states (T +- dT at fixed e, e (1 +- re) at
// fixed T), each [nprof][nf][nlev] as k_absorb writes them -- absorption is a LOCAL function of (p, T, e), so its
// partial derivatives are central differences of five evaluations per level, whatever the number of levels.
// Everything downstream is differentiated analytically:
//   tau_l = (LM(aw_l, aw_{l-1}) + LM(ad_l, ad_{l-1})) dz_l am,
//   B_tot = sum_l c_l T_{l-1} + B_cosmic T_n,   c_l = (b_{l-1} + b_l E_l)(1 - E_l)/(1 + E_l),  E_l = exp(-tau_l),
//   dB_tot/dtau_l = T_{l-1} dc_l/dtau_l - (B_tot - sum_{m<=l} c_m T_{m-1})     (everything above layer l is dimmed),
//   dTB/dB_tot = hvk / (ln^2(1 + 1/B) B (B + 1)),   db/dT = b (b + 1) hvk / T^2.
// One thread per (profile, frequency, elevation): two serial walks over the levels (the first for B_tot).  An analysis
// product, not a throughput path.
// ---------------------------------------------------------------------------------------------
// log-mean layer value and its two partial derivatives, branch for branch as layer_value<true>
__device__ __forceinline__ double layer_value_grad(double x1, double x0, double& d1, double& d0, bool& neg) {
  if (x0 < 0.0 || x1 < 0.0) { neg = true; d1 = d0 = 0.0; return 0.0; }
  const double d = x1 - x0;
  if (fabs(d) < 1e-09) { d1 = 1.0; d0 = 0.0; return x1; }
  if (x0 == 0.0 || x1 == 0.0) { d1 = d0 = 0.5; return 0.5 * (x1 + x0); }
  const double sm = x1 + x0, s = d / sm;
  if (fabs(s) <= LOGMEAN_SMALL_S) {
    // L = sm/2 q(z), q = s/atanh(s), z = s^2:  dL/dx1 = q/2 + 2 s q'(z) x0/sm,  dL/dx0 = q/2 - 2 s q'(z) x1/sm
    const double z = s * s;
    const double c[10] = {-3.3333333333333333333e-01, -8.8888888888888888889e-02, -4.6560846560846560847e-02,
                          -3.0194003527336860670e-02, -2.1796804019026241248e-02, -1.6787551856334925118e-02,
                          -1.3502765051265933100e-02, -1.1203745637718733130e-02, -9.5160731945278989134e-03,
                          -8.2312065673505011548e-03};
    double q = 0.0, qp = 0.0;
    for (int k = 9; k >= 0; --k) { qp = qp * z + (k + 1) * c[k]; q = (q + c[k]) * z; }
    q += 1.0;
    d1 = 0.5 * q + 2.0 * s * qp * x0 / sm;
    d0 = 0.5 * q - 2.0 * s * qp * x1 / sm;
    return 0.5 * sm * q;
  }
  const double ln = log(x1 / x0), L = d / ln;
  d1 = (1.0 - L / x1) / ln;
  d0 = (L / x0 - 1.0) / ln;
  return L;
}

__global__ void __launch_bounds__(64)
k_tb_jacobian(const JacArgs A) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nlev = A.nlev, nf = A.nf, nang = A.nang;
  if (gid >= A.nprof * nf * nang) return;
  const int a = (int)(gid % nang);
  const int j = (int)((gid / nang) % nf);
  const int64_t prof = gid / ((int64_t)nang * nf);
  const cmodel M = (cmodel)A.M;
  const double qnan = __builtin_nan("");
  const int64_t orow = ((prof * nang + a) * nf + j);
  double* o_t = A.dtb_dt + orow * nlev; double* o_e = A.dtb_de + orow * nlev; double* o_z = A.dtb_ddz + orow * nlev;
  const int64_t arow = (prof * nf + j) * nlev;
  const double* z = A.z + prof * nlev; const double* t = A.t + prof * nlev;
  const double am = A.airmass[a];
  const double f = A.frq[j];
  const double hvk = f * (1e9 * M->planck_h / M->boltzmann_k);
  bool bad = false;
  for (int l = 0; l < nlev; ++l)
    bad = bad || isnan(z[l]) || isnan(t[l]) || isnan(A.a[0][0][arow + l]) || isnan(A.a[0][1][arow + l]);
  auto blank = [&](uint8_t flag) {
    A.tb[orow] = qnan;
    for (int l = 0; l < nlev; ++l) { o_t[l] = qnan; o_e[l] = qnan; o_z[l] = qnan; }
    if (flag != 1) A.valid[prof] = flag;
  };
  if (bad) { blank(0); return; }
  const double* aw = A.a[0][0] + arow; const double* ad = A.a[0][1] + arow;
  // ---- walk 1: B_tot ----
  bool neg = false;
  double Btot = 0.0, T = 1.0;
  {
    double bprev = 1.0 / (exp(hvk / t[0]) - 1.0);
    for (int l = 1; l < nlev; ++l) {
      double g1, g0;
      const double dz = (z[l] - z[0]) - (z[l - 1] - z[0]);
      const double tau = (layer_value_grad(aw[l], aw[l - 1], g1, g0, neg) * dz + layer_value_grad(ad[l], ad[l - 1], g1, g0, neg) * dz) * am;
      const double E = exp(-tau);
      const double bl = 1.0 / (exp(hvk / t[l]) - 1.0);
      const double c = (bprev + bl * E) / (1.0 + E) * T * (1.0 - E);
      Btot += c;
      o_z[l] = c;                                                 // (scratch until walk 2: c_l T_{l-1})
      T *= E;
      bprev = bl;
    }
  }
  if (neg) { blank(2); return; }
  const double bbg = 1.0 / (exp(hvk / M->t_cosmic) - 1.0);
  const bool with_bg = T > TRANS_MIN;
  if (with_bg) Btot += bbg * T;
  const double Lg = log(1.0 + 1.0 / Btot);
  A.tb[orow] = hvk / Lg;
  const double dTB_dB = hvk / (Lg * Lg * Btot * (Btot + 1.0));
  if (isnan(am)) { blank(1); return; }                          // a NaN elevation: its rows are NaN, the profile stays valid
  // the radiance reaching the antenna from above each layer, sum_{m > l} c_m T_{m-1} + the cosmic term, summed from the
  // top down into o_z[l] (B_tot - S_l would cancel to ~eps B_tot where it is tiny, at levels an opaque path hides)
  {
    double above = with_bg ? bbg * T : 0.0;
    for (int l = nlev - 1; l >= 1; --l) { const double c = o_z[l]; o_z[l] = above; above += c; }
  }
  // ---- walk 2: derivatives ----
  const double inv2dT = 0.5 / A.dT;
  auto dA = [&](int species, int lvl, bool wrt_e) {             // d(absorption)/dT or /de at a level, central difference
    const double hi = A.a[wrt_e ? 3 : 1][species][arow + lvl], lo = A.a[wrt_e ? 4 : 2][species][arow + lvl];
    return wrt_e ? (hi - lo) / (2.0 * A.de[prof * nlev + lvl]) : (hi - lo) * inv2dT;
  };
  double Tm = 1.0;
  double b0 = 1.0 / (exp(hvk / t[0]) - 1.0);
  double acc_t = 0.0, acc_e = 0.0;                              // contributions to level l-1 collected so far
  o_z[0] = 0.0;
  for (int l = 1; l < nlev; ++l) {
    double w1, w0, d1, d0;
    const double dz = (z[l] - z[0]) - (z[l - 1] - z[0]);
    const double Lw = layer_value_grad(aw[l], aw[l - 1], w1, w0, neg), Ld = layer_value_grad(ad[l], ad[l - 1], d1, d0, neg);
    const double tau = (Lw * dz + Ld * dz) * am;
    const double E = exp(-tau);
    const double b1 = 1.0 / (exp(hvk / t[l]) - 1.0);
    const double opE = 1.0 + E, omE = 1.0 - E;
    const double dc_dtau = E * (2.0 * b0 + 2.0 * b1 * E - b1 + b1 * E * E) / (opE * opE);
    // everything above layer l (later layers and the cosmic term, o_z[l] from the top-down sum) is dimmed by E_l
    const double g = dTB_dB * (Tm * dc_dtau - o_z[l]);                          // dTB/dtau_l
    const double gk = g * am * dz;
    // level l-1 (lower end of the layer) and level l (upper end)
    acc_t += gk * (w0 * dA(0, l - 1, false) + d0 * dA(1, l - 1, false)) + dTB_dB * Tm * (omE / opE) * (b0 * (b0 + 1.0) * hvk / (t[l - 1] * t[l - 1]));
    acc_e += gk * (w0 * dA(0, l - 1, true) + d0 * dA(1, l - 1, true));
    o_t[l - 1] = acc_t; o_e[l - 1] = acc_e;
    acc_t = gk * (w1 * dA(0, l, false) + d1 * dA(1, l, false)) + dTB_dB * Tm * (E * omE / opE) * (b1 * (b1 + 1.0) * hvk / (t[l] * t[l]));
    acc_e = gk * (w1 * dA(0, l, true) + d1 * dA(1, l, true));
    // dTB / d(thickness of layer l) [K/km]: tau_l = m (Lw + Ld) dz_l is linear in dz_l, so this holds at dz_l = 0 too
    o_z[l] = g * am * (Lw + Ld);
    Tm *= E;
    b0 = b1;
  }
  o_t[nlev - 1] = acc_t; o_e[nlev - 1] = acc_e;
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

hipError_t launch_ray_paths(const double* z, const double* p, const double* t, const double* rh, int64_t nprof, int nlev,
                            const double* elev_deg, int nang, double* amf, uint8_t* duct, hipStream_t st) {
  hipLaunchKernelGGL(k_ray_paths, dim3((unsigned)nprof), dim3(lanes_for(nlev)), 0, st, z, p, t, rh, nlev, elev_deg, nang, amf,
                     duct);
  return hipGetLastError();
}

hipError_t launch_tb_jacobian(const JacArgs& a, hipStream_t st) {
  const int64_t nthreads = a.nprof * a.nf * a.nang;
  hipLaunchKernelGGL(k_tb_jacobian, dim3((unsigned)((nthreads + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_selftest_math(const double* x, const double* y, double* out_exp, double* out_log, double* out_div,
                                double* out_div1, int n, hipStream_t st) {
  hipLaunchKernelGGL(k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, st, x, y, out_exp, out_log, out_div, out_div1, n);
  return hipGetLastError();
}

}  // namespace mwrt
