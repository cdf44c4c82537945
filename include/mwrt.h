/*
 * mwrt.h -- C ABI of the MI355X-native line-by-line microwave forward operator.
 *
 * Drop-in boundary for ONE path of apschera2023uzk/MWR_fast_forward_operators_and_LBLs:
 * the pyrtlib LBL call made by python_src/proc/PyRTlib_processing.py:123-127
 *
 *     rte = TbCloudRTE(z[::-1], p[::-1], t[::-1], rh[::-1], frqs, ang)   (:123)
 *     rte.init_absmdl(mdl)                                               (:124)
 *     rte.satellite = False                                              (:125)
 *     df = rte.execute(); tbs[i,:,k,j] = df["tbtotal"].values            (:126-127)
 *
 * The reference has no FFI layer of its own: these entry points are
 * what a ctypes stub placed behind that Python call surface binds.
 * Plain pointers and sizes only; the library never throws across the boundary; every
 * function returns an mwrt_status (0 = ok, <0 = error, text via mwrt_last_error()).
 *
 * Array conventions (all float64, C-contiguous, caller-owned):
 *   profiles   [nprof][nlev], level 0 = ground, level nlev-1 = top -- what TbCloudRTE sees
 *              after the wrapper's [::-1] (:123); z in km, p in hPa, T in K, rh as fraction
 *              (:109-114).
 *   frq_ghz    [nf]    (:87-88)  Frequencies: the absorption models hold for 1 ... 1000 GHz, and that is the range
 *              the kernels' arithmetic is bounded for (the far-line sums carry products of up to twenty line
 *              denominators, ~f^80).  The range is a precondition, not checked: up to about 1.6 THz the
 *              stated headroom still holds, from about 7 THz these products overflow and TBs come out inf / NaN
 *              with valid = 1.
 *   elev_deg   [nang]  ELEVATION angles in (0, 180), 90 = zenith (:106, :37); the path is
 *              plane-parallel (air mass 1/sin elev), other values are MWRT_ERR_INVALID_ARGUMENT
 *   tb_out     [nprof][nang][nf]  == pyrtlib's DataFrame row order (angle-major) per profile
 *   valid_out  [nprof] 1 = ok; 0 = NaN in the inputs of that profile (the wrapper's
 *              check_for_nans, :71-79, :117-119: outputs stay NaN); 2 = negative absorption
 *              met in the layer integration (pyrtlib raises ValueError there); 3 = a ray of this
 *              profile was trapped (ducting) while ray tracing (that angle's outputs are NaN).
 *
 * NaN rules (check_for_nans is evaluated per (time, Crop, elevation), :101-119):
 *   NaN in a profile's z/p/T/rh   -> that profile's outputs NaN, valid = 0;
 *   NaN in elev_deg[k]            -> only the [:, k, :] rows are NaN (the reference skips that k
 *                                    alone, :106, :117); the other angles are computed and valid
 *                                    stays 1 -- valid describes the profile's own data;
 *   NaN in frq_ghz (or every elevation NaN) -> every output NaN, valid = 0 (frqs is shared by all
 *                                    calls of the wrapper, :87-88).
 *
 * Reproducibility: results are deterministic for a given call.  The kernels process the
 * frequencies in chunks (14 or 16 per workgroup) and choose per chunk between algebraically
 * equal forms of a line's denominator (polynomial in f^2 away from line centres, direct
 * detunings next to them), so the TB of one frequency may differ by <= 1e-8 K depending on
 * which other frequencies share its call.  Likewise the layer integration picks, per wave of
 * (frequency, elevation) pairs, between two algebraically equal forms of a layer's emission
 * (thin layers: series, no division), so a TB may differ by <= 1e-10 K depending on which
 * other elevations share its call.  Against the 1e-6 K parity bar both are invisible.
 *
 * Streams: the *_device entry points are asynchronous on `stream`:
 *   NULL               the context's own stream (hipStreamNonBlocking: NOT ordered with the
 *                      legacy default stream -- synchronise with mwrt_synchronize(ctx, NULL));
 *   MWRT_STREAM_LEGACY the caller's legacy default stream (hipStream_t 0, what
 *                      torch.cuda.current_stream().cuda_stream reads as 0);
 *   anything else      that hipStream_t.
 * Work is ordered on that stream like any kernel launch; consumers on other streams need an
 * event.  frq_ghz / elev_deg are host arrays: the first call with new values makes an immutable
 * device copy (a short host-side wait on the context's stream); later calls with the same values
 * neither allocate nor synchronise, which is what makes the call hipGraph-capturable after one
 * warm-up call.
 */
#ifndef MWRT_H
#define MWRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MWRT_VERSION 301          /* 0.3.1: + mwrt_set_chunk_width; 0.3.0: layer-optical-depth two-kernel form (mwrt_layer_tau_*, mwrt_tb_from_layer_tau_device) */
#define MWRT_MAX_H2O_LINES 32
#define MWRT_MAX_O2_LINES 64
#define MWRT_MAX_X_LINES 64       /* lines of the extra trace species (ozone) */
#define MWRT_MAX_LEVELS 1024      /* one lane per level, one workgroup per profile */
#define MWRT_MAX_ANGLES 64
#define MWRT_STREAM_LEGACY ((void*)(intptr_t)-1)   /* `stream` value meaning hipStream_t 0 */

typedef enum {
  MWRT_OK = 0,
  MWRT_ERR_INVALID_ARGUMENT = -1,
  MWRT_ERR_NO_DEVICE = -2,
  MWRT_ERR_HIP = -3,
  MWRT_ERR_OUT_OF_MEMORY = -4,
  MWRT_ERR_UNSUPPORTED = -5
} mwrt_status;

/* Replaces pyrtlib's process-global model state set by init_absmdl(str) (:124): an explicit,
 * immutable table record.  Field-for-field image of spectroscopy.ModelTables (Python host). */
typedef struct mwrt_model_desc {
  int32_t n_h2o, n_o2;
  int32_t h2o_shift_mode;   /* 0 none (R98); 2 air+self shift with ln-T coefficients (R17+) */
  int32_t o2_mix_mode;      /* 0 first order on total pressure (R98/R17); 1 second order on den (R19+) */
  int32_t o2_line1_dens;    /* R98: 118.75-GHz width uses DENS (first-order mixing mode only) */
  int32_t n2_fdep;          /* absn2 frequency-dependence factor on/off */
  int32_t n2_ptot;          /* 1: N2 at total pressure (pre-2019, folded into the O2 routine) */
  int32_t liq_mode;         /* cloud liquid (opt-in): 0 Liebe 1991 / MPM93 double Debye; 1 Rosenkranz 2015 */
  double h2o_reftcon, h2o_reftline, h2o_cf, h2o_xcf, h2o_cs, h2o_xcs, h2o_pvap_div, h2o_den_coef;
  double o2_x, o2_wb300, o2_pvap_div, o2_wv_factor, o2_nonres, o2_coef;
  double n2_l, n2_m, n2_n;
  double t_cosmic, planck_h, boltzmann_k;
  double h2o_fl[MWRT_MAX_H2O_LINES], h2o_s1[MWRT_MAX_H2O_LINES], h2o_b2[MWRT_MAX_H2O_LINES];
  double h2o_w0[MWRT_MAX_H2O_LINES], h2o_x[MWRT_MAX_H2O_LINES];
  double h2o_w0s[MWRT_MAX_H2O_LINES], h2o_xs[MWRT_MAX_H2O_LINES];
  double h2o_sh[MWRT_MAX_H2O_LINES], h2o_xh[MWRT_MAX_H2O_LINES];
  double h2o_shs[MWRT_MAX_H2O_LINES], h2o_xhs[MWRT_MAX_H2O_LINES];
  double h2o_aair[MWRT_MAX_H2O_LINES], h2o_aself[MWRT_MAX_H2O_LINES];
  double h2o_w2[MWRT_MAX_H2O_LINES], h2o_xw2[MWRT_MAX_H2O_LINES];
  double h2o_w2s[MWRT_MAX_H2O_LINES], h2o_xw2s[MWRT_MAX_H2O_LINES];
  double h2o_d2[MWRT_MAX_H2O_LINES], h2o_d2s[MWRT_MAX_H2O_LINES];
  double o2_f[MWRT_MAX_O2_LINES], o2_s300[MWRT_MAX_O2_LINES], o2_be[MWRT_MAX_O2_LINES];
  double o2_w300[MWRT_MAX_O2_LINES], o2_y0[MWRT_MAX_O2_LINES], o2_y1[MWRT_MAX_O2_LINES];
  double o2_g0[MWRT_MAX_O2_LINES], o2_g1[MWRT_MAX_O2_LINES];
  double o2_dnu0[MWRT_MAX_O2_LINES], o2_dnu1[MWRT_MAX_O2_LINES];
  /* Extra trace species (ozone): pyrtlib's TbCloudRTE(..., o3n=...) adds O3AbsModel.o3_absorption to the dry
   * absorption [EXT; Rosenkranz o3abs].  The reference builds an O3 profile for the sibling model
   * (python_src/proc/ARMS_gb_processing.py:94-99) and leaves o3n at None on the LBL path, so this is opt-in
   * (mwrt_tb_options.o3n) and DATA-FREE here: the line list could not be restated offline; n_x = 0 means "no table"
   * and a call that passes o3n is refused.  tools/export_pyrtlib_tables.py dumps pyrtlib's list into these fields.
   *   alpha_x [Np/km] = x_coef * n [molecules m-3] * qvinv * ti^2.5 * sum_k S1_k exp(B_k (1 - ti)) (f/FL_k)^2
   *                     * [ w_k / ((f - FL_k)^2 + w_k^2) + w_k / ((f + FL_k)^2 + w_k^2) ],
   *   ti = x_reft / T,  qvinv = 1 - exp(-x_qvib_t / T)  (1 if x_qvib_t <= 0),
   *   w_k = 0.5346 wc + sqrt(0.2166 wc^2 + 0.6931 bd^2)   (Voigt half width, Olivero & Longbothum 1977),
   *   wc = W_k p ti^X_k  (p total, hPa),  bd = 4.3e-7 sqrt(T / x_mass) FL_k  (Doppler 1/e half width). */
  int32_t n_x;
  int32_t x_reserved;
  double x_reft, x_qvib_t, x_mass, x_coef;
  double x_fl[MWRT_MAX_X_LINES], x_s1[MWRT_MAX_X_LINES], x_b[MWRT_MAX_X_LINES];
  double x_w[MWRT_MAX_X_LINES], x_x[MWRT_MAX_X_LINES];
} mwrt_model_desc;

/* Optional by-products of execute() (the other DataFrame columns pyrtlib returns; the
 * reference reads only "tbtotal", :127).  Any pointer may be NULL. */
typedef struct mwrt_tb_extras {
  double* tbatm;    /* [nprof][nang][nf] */
  double* tmr;      /* [nprof][nang][nf] */
  double* tauwet;   /* [nprof][nang][nf] slant-path opacity, Np */
  double* taudry;   /* [nprof][nang][nf] */
  double* taulay;   /* [nprof][nf][nlev] ZENITH layer optical depth (wet+dry+ice+liquid), entry 0 = 0 */
  double* tauliq;   /* [nprof][nang][nf] cloud liquid opacity (0 unless mwrt_tb_options.denliq is given) */
  double* tauice;   /* [nprof][nang][nf] cloud ice opacity */
} mwrt_tb_extras;

/* Physics pyrtlib offers and the reference leaves at its defaults (TbCloudRTE(..., ray_tracing=False,
 * cloudy=False); the author prints rte.cloudy at old_processing.py:558-563).  STRICTLY OPT-IN: a NULL
 * options pointer, or all-zero options, is the reference's clear-sky plane-parallel path bit for bit.
 *   denliq / denice  cloud liquid / ice density profiles [nprof][nlev] in g m-3 (what init_cloudy takes);
 *                    the upstream producer stores kg/kg: python_src/preproc/derive_cloud_water.py:68-142,
 *                    preprocessing4all.py:811-812, :1199-1200 ("Level_Liquid", "Level_Ice").
 *                    RTEquation.cloudy_absorption + exponential_integration(zeroflg = False).
 *   o3n              ozone number density profiles (see mwrt_model_desc.n_x): opt-in, and refused without a line table.
 *   ray_tracing      != 0: spherical refracted slant paths (RTEquation.refractivity, Thayer 1974, and
 *                    RTEquation.ray_tracing, TBMODEL RAYTRAC) instead of dz / sin(elev) -- matters for the
 *                    4.2 ... 8.4 degree elevations of PyRTlib_processing.py:37.
 * On the *_device entry point denliq / denice are DEVICE pointers. */
typedef struct mwrt_tb_options {
  const double* denliq;
  const double* denice;
  int32_t ray_tracing;
  int32_t reserved0;
  const double* o3n;       /* ozone number density [nprof][nlev], molecules m-3 (pyrtlib's o3n), or NULL; needs a model
                              with n_x > 0 (else MWRT_ERR_UNSUPPORTED); added to the dry absorption of every level */
} mwrt_tb_options;

typedef struct mwrt_context mwrt_context;   /* one per (host thread, GPU): device, stream, workspace */
typedef struct mwrt_model mwrt_model;       /* device-resident copy of an mwrt_model_desc */

int mwrt_version(void);
/* sizeof(mwrt_model_desc) as compiled into the library (binding self-check). */
size_t mwrt_model_desc_size(void);
/* Number of usable HIP devices; 0 when there is no GPU / driver (never an error). */
int mwrt_device_count(void);
/* Thread-local text of the last failure on this thread ("" if none). */
const char* mwrt_last_error(void);

int mwrt_create(int device_id, mwrt_context** out);
int mwrt_destroy(mwrt_context* ctx);
int mwrt_model_create(mwrt_context* ctx, const mwrt_model_desc* desc, mwrt_model** out);
int mwrt_model_destroy(mwrt_context* ctx, mwrt_model* model);

/* TbCloudRTE(...).execute() for a batch of profiles; HOST buffers, synchronous.
 * Replaces the triple loop + 4 x execute() of PyRTlib_processing.py:99-151 for one model. */
int mwrt_tb_batch(mwrt_context* ctx, const mwrt_model* model,
                  int64_t nprof, int32_t nlev,
                  const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                  int32_t nf, const double* frq_ghz,
                  int32_t nang, const double* elev_deg,
                  double* tb_out, uint8_t* valid_out, const mwrt_tb_extras* extras);

/* Same, on DEVICE buffers (profiles, tb_out, valid_out and the extras already in HBM),
 * asynchronous on `stream` (a hipStream_t; NULL / MWRT_STREAM_LEGACY: see "Streams" above).
 * frq_ghz and elev_deg stay small host arrays.  This is the entry bench.py times. */
int mwrt_tb_batch_device(mwrt_context* ctx, const mwrt_model* model,
                         int64_t nprof, int32_t nlev,
                         const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                         const double* d_rh_frac,
                         int32_t nf, const double* frq_ghz,
                         int32_t nang, const double* elev_deg,
                         double* d_tb_out, uint8_t* d_valid_out, const mwrt_tb_extras* d_extras,
                         void* stream);

/* mwrt_tb_batch / mwrt_tb_batch_device with the opt-in physics of mwrt_tb_options (NULL = none). */
int mwrt_tb_batch_opt(mwrt_context* ctx, const mwrt_model* model,
                      int64_t nprof, int32_t nlev,
                      const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                      int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                      double* tb_out, uint8_t* valid_out, const mwrt_tb_extras* extras,
                      const mwrt_tb_options* options);
int mwrt_tb_batch_opt_device(mwrt_context* ctx, const mwrt_model* model,
                             int64_t nprof, int32_t nlev,
                             const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                             const double* d_rh_frac,
                             int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                             double* d_tb_out, uint8_t* d_valid_out, const mwrt_tb_extras* d_extras,
                             const mwrt_tb_options* d_options, void* stream);

/* Several absorption models over the SAME profiles in one launch (and one host->device copy): what
 * the wrapper does four times per profile, R20/R24/R17/R98 (PyRTlib_processing.py:121-151).
 * nmodels <= 8; tb_out [nmodels][nprof][nang][nf], valid_out [nmodels][nprof]. */
int mwrt_tb_batch_multi(mwrt_context* ctx, int32_t nmodels, const mwrt_model* const* models,
                        int64_t nprof, int32_t nlev,
                        const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                        int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                        double* tb_out, uint8_t* valid_out);
int mwrt_tb_batch_multi_device(mwrt_context* ctx, int32_t nmodels, const mwrt_model* const* models,
                               int64_t nprof, int32_t nlev,
                               const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                               const double* d_rh_frac,
                               int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                               double* d_tb_out, uint8_t* d_valid_out, void* stream);

/* RTEquation.clearsky_absorption for a batch: awet, adry [nprof][nf][nlev] in Np/km
 * (exposes kernel K1 alone, for parity tests and the roofline measurement). HOST buffers. */
int mwrt_absorption_batch(mwrt_context* ctx, const mwrt_model* model,
                          int64_t nprof, int32_t nlev,
                          const double* p_hpa, const double* t_k, const double* rh_frac,
                          int32_t nf, const double* frq_ghz,
                          double* awet_out, double* adry_out);
int mwrt_absorption_batch_device(mwrt_context* ctx, const mwrt_model* model,
                                 int64_t nprof, int32_t nlev,
                                 const double* d_p_hpa, const double* d_t_k, const double* d_rh_frac,
                                 int32_t nf, const double* frq_ghz,
                                 double* d_awet_out, double* d_adry_out, void* stream);

/* Frequencies per workgroup of the fused TB kernel: 0 = automatic (default), or 8 / 14 / 16.  Automatic: 14 for channel lists
 * that are a multiple of 14 (the HATPRO list: one workgroup per profile, every per-(level, line) quantity computed once), 16
 * otherwise, whatever the batch size -- so a profile's results do not depend on the batch it arrives in, bit for bit.
 * 8 is the latency setting for small batches: two workgroups per 14-channel profile (MI355X, seven elevations: one profile
 * 58 instead of 75 us, 256 profiles 61 instead of 76, 512 profiles 77 instead of 83; slower from ~600 profiles up).  The width
 * changes the grouping of the line sums, so results move by ~1e-13 relative between widths. */
int mwrt_set_chunk_width(mwrt_context* ctx, int width);

/* How a fine spectral grid is evaluated: 0 = automatic (windowed when the frequency list qualifies: >= 128 strictly
 * increasing frequencies whose 128-frequency windows each span <= 6 GHz, <= 505 levels, LDS permitting), 1 = always every
 * line at every frequency, 2 = windowed or MWRT_ERR_UNSUPPORTED.  Windowed: the lines >= 4 GHz beyond a window are summed
 * at 16 Chebyshev nodes of the window and interpolated (error <= 1e-10 of the line sum), the others are evaluated
 * directly; results agree with mode 1 to ~1e-10 relative.
 * Governs mwrt_absorption_batch[_device] and mwrt_layer_tau_batch_device (modes 0, 1, 2 as above), and the TB entry
 * points' automatic fine-grid path (windowed K1 -> layer optical depth in HBM -> RTE kernel): mode 1 switches that
 * path off (one fused kernel, every line at every frequency); modes 0 and 2 both leave it automatic -- a TB call is
 * never refused for its frequency list. */
int mwrt_set_absorption_mode(mwrt_context* ctx, int mode);

/* The second half of execute() on its own: layer optical depths (exponential_integration, zeroflg = True) +
 * downwelling Planck-space RTE (planck, bright) from absorption coefficients ALREADY in HBM, laid out as
 * mwrt_absorption_batch_device writes them (awet, adry [nprof][nf][nlev], Np/km).  Together the two calls are
 * the K1 -> alpha -> K2 two-kernel form of the fine-grid configuration (BASELINE configs[4]: alpha is 3.6 GB
 * per GPU, written once and read once); it is also the entry for callers who bring their own absorption.
 * `model` supplies the RTE constants only (t_cosmic, h, k).  DEVICE buffers; valid as for mwrt_tb_batch
 * (0 also for a NaN absorption coefficient). */
int mwrt_tb_from_absorption_device(mwrt_context* ctx, const mwrt_model* model,
                                   int64_t nprof, int32_t nlev,
                                   const double* d_z_km, const double* d_t_k,
                                   int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                   const double* d_awet, const double* d_adry,
                                   double* d_tb_out, uint8_t* d_valid_out, void* stream);

/* The fine-grid two-kernel form with the LAYER OPTICAL DEPTH as the hand-over (what the TB entry points run
 * automatically on window-eligible frequency lists; BASELINE configs[4]: 1.8 GB per GPU written once, read once):
 *   mwrt_layer_tau_batch_device   clearsky_absorption + exponential_integration(zeroflg = True) on wet and dry,
 *                                 summed [EXT, reached from PyRTlib_processing.py:126]: zenith layer optical depth
 *                                 d_tau_out [nprof][nlev][tau_pitch] in Np (entry [.][0][.] = 0; 8 B per (profile,
 *                                 level, frequency), FREQUENCY fastest), d_valid_out [nprof] as for mwrt_tb_batch
 *                                 (a profile flagged 0 or 2 has NaN rows).  tau_pitch = doubles between consecutive
 *                                 levels: a multiple of 16, >= mwrt_layer_tau_pitch(nf) (= nf rounded up to 16);
 *                                 columns [nf, tau_pitch) are scratch.  nlev <= 1009.
 *   mwrt_tb_from_layer_tau_device RTEquation.planck (from_sat = False) + bright [EXT]: TBs [nprof][nang][nf] from such
 *                                 an array (tau_pitch >= nf), T [nprof][nlev] and d_valid [nprof] (1 = integrate,
 *                                 anything else = that profile's TBs are NaN).  `model` supplies h, k, t_cosmic.
 * DEVICE buffers, asynchronous on `stream`.
 * Specified range of the two RTE entries (this one and mwrt_tb_from_absorption_device): every layer optical depth times
 * every air mass FINITE and at most 1e6 in magnitude (beyond about 700 the layer's transmission is 0 and the path
 * below it is all that is seen).  Within it the TBs are held to the 50-digit reference (tests/test_rte_columns.py); a
 * NaN optical depth makes the TBs of its own (profile, frequency) NaN and touches nothing else.  An infinite optical
 * depth, or a product beyond about 1e40, is outside it: the exponential's range reduction then yields NaN or inf instead
 * of 0 -- confined to the outputs of that (profile, frequency), but not the opaque-layer answer. */
int mwrt_layer_tau_pitch(int32_t nf);
int mwrt_layer_tau_batch_device(mwrt_context* ctx, const mwrt_model* model,
                                int64_t nprof, int32_t nlev,
                                const double* d_z_km, const double* d_p_hpa, const double* d_t_k, const double* d_rh_frac,
                                int32_t nf, const double* frq_ghz,
                                double* d_tau_out, int32_t tau_pitch, uint8_t* d_valid_out, void* stream);
int mwrt_tb_from_layer_tau_device(mwrt_context* ctx, const mwrt_model* model,
                                  int64_t nprof, int32_t nlev,
                                  const double* d_tau, int32_t tau_pitch, const double* d_t_k,
                                  int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                  const uint8_t* d_valid, double* d_tb_out, void* stream);

/* K-matrix of the operator in ONE call: the block the reference parses out of RTTOV-gb's K run
 * (python_src/proc/RTTOV_gb_processing.py:286-300, :418-432: dTB/dT, dTB/dq per level and channel).  Partial derivatives
 * of every TB with respect to the LBL inputs of each level, [nprof][nang][nf][nlev]:
 *   dtb_dt   K/K      d TB / d T_i       at fixed vapour pressure e_i, pressure and heights
 *   dtb_de   K/hPa    d TB / d e_i       (e = rh * es(T), Goff-Gratch) at fixed T_i
 *   dtb_ddz  K/km     d TB / d (z_i - z_{i-1})   thickness of the layer below level i (entry 0 = 0)
 * Clear sky, plane-parallel.  HOST buffers, synchronous; tb_out as mwrt_tb_batch; valid_out as there (0 / 2: that
 * profile's outputs are NaN).
 * This is the tangent-linear path of the device K-matrix (below) on host buffers: exactly
 * mwrt_tb_jacobian_batch_vars with options = NULL, vars = NULL, no cloud rows and dtb_ddz required -- one implementation,
 * the same bits.  The absorption derivatives are exact (mwrt_absorption_tl_batch_device), the layer rule
 * (exponential_integration), the Planck-space recursion and bright() are differentiated analytically (adjoint), so the
 * cost is a few forward runs whatever nlev -- not the 3 nlev + 1 forward runs of a brute-force K-matrix.
 * Until the device path replaced it, this entry differenced the absorption (T +- 0.01 K, e (1 +- 1e-4)) in a kernel of
 * its own.  What moved when that kernel was retired (MWRT_VERSION stays 301: symbol, signature, units, layouts and status
 * codes are unchanged):
 *   values     dtb_dt and dtb_de are the exact derivative instead of a central difference of it: they moved by the old
 *              step error, <= 2e-5 of a row (<= 1e-3 of a row where the e-step sat at its 1e-7 hPa floor, and arbitrary
 *              where +- 0.01 K straddled a branch of the absorption); dtb_ddz and tb_out moved by rounding only;
 *   mode       independent of mwrt_set_absorption_mode, like every K-matrix entry (under forced mode 2 a short frequency
 *              list used to be MWRT_ERR_UNSUPPORTED here; now it computes);
 *   memory     no profile batching: everything is staged at once (inputs, tb and three rows in a buffer of the call's
 *              own, freed on return) next to the context's workspace of 48 B per (profile, frequency, level), which stays
 *              allocated; nprof * nf > 2^31 - 1 is MWRT_ERR_UNSUPPORTED, as for mwrt_tb_jacobian_batch_vars;
 *   nprof = 0  returns MWRT_OK once sizes and pointers are checked, as mwrt_tb_jacobian_batch_vars does (a NaN frequency
 *              used to be looked for first). */
int mwrt_tb_jacobian_batch(mwrt_context* ctx, const mwrt_model* model,
                           int64_t nprof, int32_t nlev,
                           const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                           int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                           double* tb_out, double* dtb_dt, double* dtb_de, double* dtb_ddz, uint8_t* valid_out);

/* The device K-matrix path.  Plane-parallel; clear sky, or cloud liquid / ice through
 * mwrt_tb_jacobian_batch_opt_device.  All entries are independent of
 * mwrt_set_absorption_mode and mwrt_set_chunk_width: the absorption is summed over every line at every frequency.
 *
 * mwrt_absorption_tl_batch_device: clearsky_absorption and its exact partial derivatives (tangent-linear, not finite
 *   differences), all [nprof][nf][nlev]: d_awet, d_adry in Np/km (equal to mwrt_absorption_batch_device under absorption
 *   mode 1 to rounding); d_dawet_dt, d_dadry_dt in Np/km/K at fixed vapour pressure e; d_dawet_de, d_dadry_de in
 *   Np/km/hPa at fixed T (e = rh * es(T), Goff-Gratch).  At a dry level (e = 0) the e-derivative is the right-sided one.
 *   Where the O2 term is clamped at 0 its tangent is 0.  NaN inputs give NaN outputs.  DEVICE buffers, asynchronous on
 *   `stream`. */
int mwrt_absorption_tl_batch_device(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                    const double* d_p_hpa, const double* d_t_k, const double* d_rh_frac,
                                    int32_t nf, const double* frq_ghz,
                                    double* d_awet, double* d_adry, double* d_dawet_dt, double* d_dawet_de,
                                    double* d_dadry_dt, double* d_dadry_de, void* stream);

/* The K-matrix on caller-owned HBM -- what mwrt_tb_jacobian_batch stages its host buffers into: the same outputs,
 * layouts, units and valid flags, computed from the tangent-linear absorption above and the adjoint of the layer rule +
 * RTE (no finite differences).  DEVICE buffers
 * (d_tb [nprof][nang][nf], d_dtb_* [nprof][nang][nf][nlev], d_valid [nprof]), asynchronous on `stream`; frq_ghz and
 * elev_deg are host arrays as for the other *_device entries.  Everything is decided on the device: a profile with a NaN
 * in z / p / T / rh (valid 0) or a negative absorption coefficient (valid 2) has NaN TBs and NaN Jacobian rows; a NaN
 * elevation blanks only its own rows.  A NaN frequency is MWRT_ERR_INVALID_ARGUMENT.  Workspace: 48 B per (profile,
 * frequency, level), owned by the context and only grown; after one warm-up call with the same shapes and frequencies a
 * call neither allocates nor synchronises (hipGraph-capturable).
 * Measured on MI355X at 1000 profiles x 14 channels x 7 elevations x 180 levels (R24), HIP events, median of 30: 0.58 ms
 * (k_absorb_tl 0.38 + k_jac_rte 0.22), 5.0x the 0.116-ms mwrt_tb_batch_device call on the same stream. */
int mwrt_tb_jacobian_batch_device(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                  const double* d_z_km, const double* d_p_hpa, const double* d_t_k, const double* d_rh_frac,
                                  int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                  double* d_tb, double* d_dtb_dt, double* d_dtb_de, double* d_dtb_ddz, uint8_t* d_valid,
                                  void* stream);

/* mwrt_tb_jacobian_batch_device under cloud: the K-matrix of the operator mwrt_tb_batch_opt_device computes with
 * d_options->denliq / denice (DEVICE pointers [nprof][nlev], g m-3; either may be NULL), and two more Jacobians,
 *   d_dtb_dliq  K per g m-3   d TB / d denliq_i        d_dtb_dice  K per g m-3   d TB / d denice_i
 * [nprof][nang][nf][nlev] each; either may be NULL (not wanted).  The T, e and thickness Jacobians carry the cloud's
 * optical depth.  All cloud work happens inside k_jac_rte: no further launch and no further workspace.
 * (MWRT_VERSION stays 301, as it did when the clear-sky device K-matrix was added: the symbol is an addition.)
 *   Refused: options->ray_tracing != 0 or options->o3n != NULL -> MWRT_ERR_UNSUPPORTED (the adjoint is plane-parallel and
 *   has no ozone tangent); d_dtb_dliq without denliq, or d_dtb_dice without denice -> MWRT_ERR_INVALID_ARGUMENT.
 *   Clear sky: d_options NULL, or both cloud pointers NULL, is mwrt_tb_jacobian_batch_device itself (which calls this
 *   entry), bit for bit; so is a call whose cloud arrays hold no positive entry (its cloud rows are all 0).  Streams,
 *   workspace, NaN-frequency handling and the no-allocation / no-synchronisation claim after one warm-up call are the clear entry's.
 *   Flags: a NaN in denliq / denice -> valid 0, every row of the profile NaN, as the forward kernel.  A negative cloud
 *   absorption coefficient -> valid 2; it can arise only per frequency (a negative frequency under ice, or a temperature
 *   far outside the liquid model's range), and the rows of the frequencies where it arises are NaN.
 * Derivative conventions -- the derivative of the branch the forward takes, as for the clear rows:
 *   aliq_i = denliq_i * kappa(T_i, f) for denliq_i > 0, else 0: d aliq / d denliq = kappa, d aliq / dT = denliq * d kappa / dT
 *     (kappa: LiqAbsModel.liquid_water_absorption per g m-3, either liq_mode, differentiated exactly);
 *   aice_i = k_ice * f * denice_i for denice_i > 0, else 0: no T tangent;
 *   a density <= 0 is "no cloud": its derivative is 0;
 *   the layer rule is exponential_integration(zeroflg = False): a layer with a zero end value has the value 0 and the
 *     partials (0, 0).  (The log-mean's own one-sided slope at a zero end is infinite: a forward difference of 1e-4 g m-3
 *     there gives 4e3 - 1.5e4 K per g m-3 and grows as the step shrinks.)  So an ISOLATED cloudy level -- both
 *     neighbours without cloud -- contributes nothing to the TBs and its row entries are all 0; cloud shows from two
 *     adjacent cloudy levels on;
 *   |x1 - x0| < 1e-9 gives the value x1 and the partials (1, 0); otherwise the log-mean partials of the clear rows;
 *   dtb_dt (fixed e) gains the liquid term; dtb_ddz is g m (Lw + Ld + Ll + Li); dtb_de keeps its form;
 *   a layer's optical depth is summed as the forward does, ((wet + dry) + ice) + liquid, so the TBs equal
 *     mwrt_tb_batch_opt_device's to 1e-8 K.
 * Not yet timed on a GPU (DESIGN.md 4.5.2 says what has been measured); k_jac_rte keeps the occupancy (5 waves/SIMD) and
 * the 0 bytes of scratch it had before the cloud path. */
int mwrt_tb_jacobian_batch_opt_device(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                      const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                                      const double* d_rh_frac,
                                      int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                      double* d_tb, double* d_dtb_dt, double* d_dtb_de, double* d_dtb_ddz,
                                      double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                                      const mwrt_tb_options* d_options, void* stream);

/* The device K-matrix in the variables a retrieval works in or a data set stores.  The INPUTS are
 * those of mwrt_tb_jacobian_batch_opt_device -- z, p, T, rh, and denliq / denice in g m-3 through the options; only the
 * variables of the returned derivatives change.  k_jac_rte changes them while each row element is still in a register:
 * no further launch, no further workspace, no second pass over the rows. */
typedef struct mwrt_jac_variables {
  int32_t humidity;  /* 0 e [hPa] (the dtb_de row); 1 rh [fraction]; 2 ppmv (e = ppmv * p / 1e6) */
  int32_t cloud;     /* 0 density [g m-3] (the dtb_dliq / dtb_dice rows); 1 mass mixing ratio [kg/kg]: den = q * 1000 * rho, rho = 100 p / (287.06 T) */
  int32_t heights;   /* 0 fixed: thickness row as it is; 1 hydrostatic: thickness folded into the T and humidity rows */
  int32_t reserved;  /* must be 0 */
} mwrt_jac_variables;

/* mwrt_tb_jacobian_batch_opt_device with `vars`.  With i the level index (0 = ground), e = rh * es(T) (Goff-Gratch) and
 * the RAW rows of that entry A_T = dtb_dt, A_e = dtb_de, Z = dtb_ddz, R_l = dtb_dliq, R_i = dtb_dice, the rows returned
 * are, applied in this order:
 *   heights = 1 (hydrostatic): the heights follow dz_i = (287.04 / 9.80665) * (Tv_i + Tv_{i-1}) / 2 * ln(p_{i-1} / p_i) / 1000 km,
 *     Tv = T (1 + 0.608 q), q = 0.622 e / (p - 0.378 e).  With c_i = (287.04 / (2 * 9.80665)) * ln(p_{i-1} / p_i) / 1000 for
 *     i >= 1, c_0 = 0, and G_i = Z_i c_i + Z_{i+1} c_{i+1} (nothing above the top level):
 *       A_T += G * (1 + 0.608 q)        A_e += G * 0.608 * T * 0.622 p / (p - 0.378 e)^2
 *     The derivative is taken at the z passed in: exact when that z obeys the rule.
 *   humidity h:  d_dtb_dh = A_e * de/dh, de/dh = 1 (e), es(T) (rh), p / 1e6 (ppmv);
 *                d_dtb_dt = A_T + A_e * (de/dT at fixed h), which is 0 for e and ppmv and rh * es'(T) for rh;
 *   cloud = 1 (kg/kg):  d_dtb_dliq = R_l * 1000 rho, d_dtb_dice = R_i * 1000 rho, and
 *                d_dtb_dt -= (R_l * denliq + R_i * denice) / T  (density falls with T at fixed mixing ratio).
 * Units: d_dtb_dt K/K at fixed h and mixing ratio / density; d_dtb_dh K/hPa, K per unit rh, or K/ppmv; cloud rows K per
 * g m-3 or K per kg/kg.
 *   d_dtb_ddz may be NULL in any mode; given, it is always the raw thickness row Z.
 *   A mode out of range, or reserved != 0 -> MWRT_ERR_INVALID_ARGUMENT.
 *   vars NULL or all zero is mwrt_tb_jacobian_batch_opt_device (which calls into this entry's implementation) bit for bit.
 *   Everything else -- refusals, NaN and valid rules (a NaN in p or rh is valid 0 as well), streams, workspace, no
 *   allocation and no synchronisation after one warm-up call -- is that entry's.  Dynamic LDS: 9 more rows of one double
 *   per lane when a mode is set (152 KiB for a cloudy call at 1024 levels).  (MWRT_VERSION stays 301: additions.) */
int mwrt_tb_jacobian_batch_vars_device(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                       const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                                       const double* d_rh_frac,
                                       int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                       double* d_tb, double* d_dtb_dt, double* d_dtb_dh, double* d_dtb_ddz,
                                       double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                                       const mwrt_tb_options* d_options, const mwrt_jac_variables* vars, void* stream);

/* The same on HOST buffers, synchronous (options->denliq / denice are host pointers): the arrays are staged through
 * device buffers of the call's own, which are freed on every return path, and the results are those of the device entry
 * bit for bit.  dtb_ddz, dtb_dliq and dtb_dice may be NULL. */
int mwrt_tb_jacobian_batch_vars(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                                int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                double* tb, double* dtb_dt, double* dtb_dh, double* dtb_ddz, double* dtb_dliq,
                                double* dtb_dice, uint8_t* valid, const mwrt_tb_options* options,
                                const mwrt_jac_variables* vars);

/* The device K-matrix along refracted spherical ray paths: the K-matrix of the operator
 * mwrt_tb_batch_opt_device computes with ray_tracing = 1.  The parameter list, layouts, units, optional pointers and the
 * meaning of `vars` are those of mwrt_tb_jacobian_batch_vars_device.  The entry always traces: options->ray_tracing is
 * not consulted.  options->o3n != NULL is MWRT_ERR_UNSUPPORTED; cloud (denliq / denice) is supported as in the
 * plane-parallel entry.  (mwrt_tb_jacobian_batch_opt_device and mwrt_tb_jacobian_batch_vars_device keep refusing
 * ray_tracing != 0.)
 *   Path factor.  The slant optical depth of layer l at elevation a is f[a][l] * tauz[l], f = ds/dz the path factor of the
 *     forward's ray tracer, formed by the same statements; d_tb equals mwrt_tb_batch_opt_device(ray_tracing = 1) to 1e-8 K.
 *   Rows.  The exact derivative of that operator: d_dtb_dt at fixed e, the humidity row at fixed T, then `vars`.  Both
 *     include the response of f to the refractive index n = Thayer(p, T, e) (p held, differentiated by hand), which enters
 *     at the level itself -- as the upper end of its layer and the lower end of the next -- and, for level 0, as the ground
 *     value n0 as well, which enters every layer of every ray outside the zenith branch.  (At 4.2 degrees and 22.24 GHz
 *     the path terms are a third of the level-0 humidity entry; above level 0 they stay below 0.5 %.)
 *   Thickness.  d_dtb_ddz[i] = d TB / d(z_i - z_{i-1}) with every other thickness and z_0 held: the levels i ... top move up
 *     together.  It is the direct term g_i f_i L_i plus the response of f_l, l >= i, to the heights of its two ends (dz, the
 *     two radii, and theta through z / rs).  Entry 0 is 0.  With heights = 1 this exact row is what is folded into the T
 *     and humidity rows.  A zero-thickness layer outside the zenith branch has f = 0 and no path tangent (the forward's
 *     branch), so its entry holds only what the layers above contribute.
 *   Zenith branch, 89 <= |elev| <= 91 degrees: f = 1 exactly and its derivative is that of the branch (0); the rows are the
 *     plane-parallel rows at air mass 1.
 *   Flags.  valid is 0 / 1 / 2 as in the plane-parallel entry, and 3 when a ray of the profile is trapped (ducting): that
 *     elevation's TB and rows are NaN, the profile's other elevations are computed.  A NaN elevation blanks only its own
 *     rows.  Flag and NaN patterns equal the forward entry's for the same inputs.
 *   Workspace, owned by the context and only grown: f and its five partials (towards n_l, n_{l-1}, n_0 and the relative
 *     heights of the layer's two ends) per (profile, elevation, level), 48 B each, plus the K path's 48 B per (profile,
 *     frequency, level).  After one warm-up call of the same shapes the call neither allocates nor synchronises.
 *   Argument checks are those of mwrt_tb_jacobian_batch_vars_device, status for status: a NULL required pointer, nlev < 2,
 *     nf < 1, a NaN frequency, nang outside 1 .. MWRT_MAX_ANGLES and a bad `vars` are MWRT_ERR_INVALID_ARGUMENT (-1);
 *     nlev > MWRT_MAX_LEVELS (1025 levels) and options->o3n are MWRT_ERR_UNSUPPORTED (-5).  Nothing is written on a refusal.
 *     A profile that is both flag 2 (negative cloud absorption) and trapped is reported as 2.
 * Timing (tools/ray_jacobian_time.py, profiles/ray_jacobian_time.json; MI355X, 1000 profiles x 180 levels x 14 channels x 7
 * elevations, HIP events, median of 30): 1.02 ms against 0.58 ms for mwrt_tb_jacobian_batch_vars_device (1.77x), cloudy with
 * (ppmv, kg/kg, hydrostatic) 1.15 ms against 0.73 ms (1.58x); k_ray_paths_tl 0.14 ms, k_absorb_tl 0.32 ms, k_jac_rte_ray
 * 0.57 ms against k_jac_rte's 0.26 ms.  (MWRT_VERSION stays 301: additions.) */
int mwrt_tb_jacobian_batch_ray_device(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                      const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                                      const double* d_rh_frac,
                                      int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                      double* d_tb, double* d_dtb_dt, double* d_dtb_dh, double* d_dtb_ddz,
                                      double* d_dtb_dliq, double* d_dtb_dice, uint8_t* d_valid,
                                      const mwrt_tb_options* d_options, const mwrt_jac_variables* vars, void* stream);

/* The same on HOST buffers, synchronous (options->denliq / denice are host pointers), staged as
 * mwrt_tb_jacobian_batch_vars stages its arrays: the staging is freed on every return path, and the results are those of
 * the device entry bit for bit. */
int mwrt_tb_jacobian_batch_ray(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                               const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                               int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                               double* tb, double* dtb_dt, double* dtb_dh, double* dtb_ddz, double* dtb_dliq,
                               double* dtb_dice, uint8_t* valid, const mwrt_tb_options* options,
                               const mwrt_jac_variables* vars);

/* One optimal-estimation (Gauss-Newton / 1D-Var) step per profile on the device (Rodgers 2000, eq. 5.10):
 *     x+ = xa + Sa K^T (K Sa K^T + Se)^-1 [ y - F(x) + K (x - xa) ]
 * for nprof profiles in one launch -- what a retrieval does next with the K-matrix of mwrt_tb_jacobian_batch_vars_device.
 * Dimensions per profile: nblk state blocks (1 .. 4; e.g. T, humidity, liquid, ice) of nlev levels each, n = nblk * nlev;
 * m observations (m = nang * nf when K comes from the Jacobian entries).  All DEVICE pointers, float64 unless stated:
 *   d_k[b], b < nblk   [nprof][m][nlev]: a Jacobian output [nprof][nang][nf][nlev] as that entry wrote it; K = [K_0 | K_1 | ...]
 *   d_x                [nprof][nblk][nlev] the current state
 *   d_xa               the prior state: [nblk][nlev] shared by all profiles, or [nprof][nblk][nlev] with xa_per_profile != 0
 *   d_sa               [n][n] prior covariance, shared, SYMMETRIC (only symmetric input is defined; cross-block terms allowed)
 *   d_se               observation-error covariance, shared: [m] variances, or [m][m] symmetric with se_full != 0
 *   d_y, d_fx          [nprof][m] the observations and the forward model at x (the tb of the Jacobian call)
 * With d = y - F(x) + K (x - xa) and G = K Sa K^T + Se = L L^T, per profile:
 *   d_x_new    [nprof][nblk][nlev]  xa + Sa K^T G^-1 d                                   required
 *   d_status   [nprof] uint8        see below                                            required
 *   d_chi2     [nprof]              d^T G^-1 d                                            optional (NULL: not wanted)
 *   d_dfs      [nprof]              tr(A) = m_used - tr(G^-1 Se), degrees of freedom for signal          optional
 *   d_post_var [nprof][nblk][nlev]  diag(Sa - Sa K^T G^-1 K Sa); NULL skips its second pass over the panels   optional
 *   d_nobs     [nprof] int32        m_used                                                optional
 * Missing observations: row i of a profile is DROPPED when y_i, fx_i, any K[i, :] or its Se entry (the variance, or any
 *   element of row i of a full Se) is not finite.  A dropped row is algebraically deleted (K row 0, d_i 0, G_ii 1, other
 *   G_i. 0); it is not counted in m_used and enters neither dfs nor chi2.  This is how a NaN elevation or a blanked
 *   channel of the K-matrix call passes through.
 * status: 1 ok;  0 x or xa of the profile not finite: every output of the profile NaN (nobs 0);  2 a Cholesky pivot fails
 *   pivot > 0 (G not positive definite, or NaN): outputs NaN (nobs = m_used);  3 no usable observation (e.g. a profile the
 *   Jacobian call flagged invalid): x_new = xa exactly, chi2 0, dfs 0, post_var = diag Sa, nobs 0.
 * Determinism: a profile's outputs depend on neither its batch-mates nor nprof (one workgroup per profile, fixed
 *   summation orders, no atomics), and x_new does not depend on which optional outputs are asked for.
 * The record starts with its own size: fields at or beyond struct_size are not read (taken as NULL), so it can grow.  The
 *   required pointers come first; a caller compiled against a shorter record that ends after d_status is served.
 * Limits: m <= MWRT_OE_MAX_M (the packed triangle of G lives in LDS), nlev <= MWRT_MAX_LEVELS, hence n <= 4096; beyond
 *   them MWRT_ERR_UNSUPPORTED with the limit in the error text.  MWRT_ERR_INVALID_ARGUMENT: a NULL required pointer,
 *   nblk outside 1 .. 4, reserved != 0, nlev < 1, m < 1, nprof < 0, struct_size too small for the required fields.
 * Streams as every *_device entry.  No workspace: the call never allocates and never synchronises.  The first launch of a
 *   size above 64 KiB of LDS (m >= 65) raises that kernel's dynamic-LDS limit once per device; a repeat call of the same
 *   size is the launch alone, so it is hipGraph-capturable after one warm-up call like the other entries (not yet
 *   exercised under capture by a test).  A struct_size that ends inside a field leaves that field unread, too.
 *   (MWRT_VERSION stays 301: additions.) */
#define MWRT_OE_MAX_M 140
typedef struct mwrt_oe_step {
  uint32_t struct_size;        /* sizeof(mwrt_oe_step) of the caller; fields beyond it are not read */
  int32_t  nblk, xa_per_profile, se_full, reserved;
  const double* d_k[4];
  const double *d_x, *d_xa, *d_sa, *d_se, *d_y, *d_fx;
  double* d_x_new;  uint8_t* d_status;                 /* required outputs */
  double *d_chi2, *d_dfs, *d_post_var;  int32_t* d_nobs;   /* optional outputs */
} mwrt_oe_step;
int mwrt_oe_step_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_step* s, void* stream);
/* sizeof(mwrt_oe_step) as compiled into the library (binding self-check). */
size_t mwrt_oe_step_size(void);

/* The same step split for Levenberg-Marquardt damping (Rodgers 2000, eq. 5.36 in the m-form).  With
 * dx = x - xa, r = y - F(x) and a damping factor gamma >= 0 per profile,
 *     x+ = xa + gamma / (1 + gamma) dx + Sa K^T u,     (K Sa K^T + (1 + gamma) Se) u = r + K dx / (1 + gamma)
 * and gamma = 0 is mwrt_oe_step_device.  G0 = K Sa K^T, r and K dx depend on x alone and are all but 1 % of the step's
 * arithmetic: linearise once per accepted state, solve once per trial gamma.
 *   mwrt_oe_lm_prepare_device   the linearisation at x: the row rule, r, K dx and G0, written to caller-owned buffers
 *   mwrt_oe_lm_solve_device     one damped trial x+ on a linearisation, with gamma per profile
 *   mwrt_oe_cost_device         J = r^T (Se,kept)^-1 r + dx^T Sa^-1 dx at a state, on the rows of a linearisation
 * One record, mwrt_oe_lm, serves the three.  Inputs are those of mwrt_oe_step (d_k, d_x, d_xa, d_sa, d_se, d_y, d_fx,
 * nblk, xa_per_profile, se_full; the same shapes, all DEVICE pointers, float64 unless stated) plus
 *   d_gamma      [nprof]                 the damping factor, finite and >= 0                       (solve)
 *   d_sa_inv     [n][n]                  Sa^-1, SYMMETRIC, formed by the caller                    (cost)
 *   d_active     [nprof] uint8, optional a profile whose flag is 0 is skipped: NONE of its outputs is touched (all three)
 * The linearisation, written by prepare and read by solve (all five) and cost (d_keep alone):
 *   d_g0         [nprof][m (m + 1) / 2]  packed lower triangle of K Sa K^T, entry (i, j <= i) at i (i + 1) / 2 + j; the rows
 *                                        and columns of a dropped observation are 0
 *   d_r, d_kdx   [nprof][m]              y - F(x) and K (x - xa); 0 in a dropped row
 *   d_keep       [nprof][m] uint8        1: the row is used.  The row rule is that of mwrt_oe_step_device
 *   d_lin_status [nprof] uint8           1 ok;  0 x or xa not finite (r, K dx and G0 NaN, keep 0);  3 no usable observation
 *                                        (r, K dx, G0 and keep 0)
 * Outputs of solve: d_x_new [nprof][nblk][nlev] and d_status [nprof] uint8 required; d_chi2 [nprof] = d^T G^-1 d with
 *   d = r + K dx / (1 + gamma), G = G0 + (1 + gamma) Se, and d_nobs [nprof] int32 optional.
 *   status: 1 ok;  0 the state not finite, now or when it was linearised (d_lin_status 0): outputs NaN, nobs 0;  2 gamma
 *   negative or not finite, or a Cholesky pivot fails pivot > 0: outputs NaN, nobs = m_used;  3 no usable observation:
 *   x_new = xa + gamma / (1 + gamma) dx (xa exactly at gamma = 0), chi2 0, nobs 0.
 * Outputs of cost: d_cost [nprof] required; d_cost_obs and d_cost_prior [nprof] (the two terms) and d_status optional.  The
 *   observation term runs over the rows d_keep names, so a trial and the state it is compared with use the same rows; with
 *   a full Se it is a Cholesky of the kept sub-matrix.  A non-finite x, xa, or y or fx in a kept row gives +inf in all
 *   three (a trial to reject, not an error: status 1).  Se (kept) not positive definite: NaN in all three and status 2.
 * Determinism, limits (m <= MWRT_OE_MAX_M, nlev <= MWRT_MAX_LEVELS: MWRT_ERR_UNSUPPORTED with the limit in the text) and
 *   streams as mwrt_oe_step_device.  MWRT_ERR_INVALID_ARGUMENT: a NULL pointer among those the call reads or must write
 *   (prepare: the inputs but d_gamma and d_sa_inv, and the linearisation; solve: d_k, d_x, d_xa, d_sa, d_se, d_gamma, the
 *   linearisation, d_x_new, d_status; cost: d_x, d_xa, d_se, d_y, d_fx, d_keep, d_sa_inv, d_cost), nblk outside 1 .. 4,
 *   reserved != 0, nlev < 1, m < 1, nprof < 0, struct_size smaller than the fixed part (24 bytes).
 * The record starts with its own size: fields at or beyond struct_size (and a field it ends inside) are taken as NULL.
 * The calls never allocate and never synchronise; each kernel's dynamic-LDS limit is raised once per device and size
 *   above 64 KiB, so a repeat call of the same size is the launch alone.  (MWRT_VERSION stays 301: additions.) */
typedef struct mwrt_oe_lm {
  uint32_t struct_size;        /* sizeof(mwrt_oe_lm) of the caller; fields beyond it are not read */
  int32_t  nblk, xa_per_profile, se_full, reserved;
  const double* d_k[4];
  const double *d_x, *d_xa, *d_sa, *d_se, *d_y, *d_fx;
  const double* d_gamma;
  double *d_g0, *d_r, *d_kdx;  uint8_t *d_keep, *d_lin_status;   /* the linearisation */
  const uint8_t* d_active;
  const double* d_sa_inv;
  double *d_cost, *d_cost_obs, *d_cost_prior;          /* outputs of cost */
  double* d_x_new;  uint8_t* d_status;  double* d_chi2;  int32_t* d_nobs;   /* outputs of solve */
} mwrt_oe_lm;
int mwrt_oe_lm_prepare_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream);
int mwrt_oe_lm_solve_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream);
int mwrt_oe_cost_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_lm* s, void* stream);
/* sizeof(mwrt_oe_lm) as compiled into the library (binding self-check). */
size_t mwrt_oe_lm_size(void);

/* What the step says about itself (Rodgers 2000, ch. 3): the gain matrix, the averaging kernel, the full
 * posterior covariance and the error budget, per profile, at gamma = 0 -- Rodgers' diagnostics are those of the undamped
 * step.  With W = K Sa [m][n] and G = K Sa K^T + Se = L L^T on the rows kept (the row rule and the statuses are those of
 * mwrt_oe_step_device: a dropped row is algebraically deleted),
 *     gain^T = G^-1 W                    [m][n]   row i is the contribution function d x^ / d y_i of observation i
 *     A      = gain K                    [n][n]   A[j][k] = sum_i gain[i][j] K[i][k], the averaging kernel d x^ / d x
 *     S^     = Sa - gain W               [n][n]   S^[j][k] = Sa[j][k] - sum_i gain[i][j] W[i][k], the posterior covariance
 *     noise_var  = diag(gain Se gain^T)  [n]      the measurement-noise part of diag S^
 *     smooth_var = diag((A - I) Sa (A - I)^T) = diag S^ - noise_var   [n]   the smoothing part
 *     avk_diag   = diag A                [n]
 *     dfs_block[b] = sum of avk_diag over block b;  their sum over b is tr(A), the step's dfs
 *   mwrt_oe_gain_device      the gain and everything that is a vector: one launch, one workgroup per profile
 *   mwrt_oe_product_device   A or S^ (or a window of their rows) from the gain entry's d_gain, d_keep and d_ksa
 * One record, mwrt_oe_char, serves both.  All DEVICE pointers, float64 unless stated.
 * mwrt_oe_gain_device reads the inputs of mwrt_oe_step (d_k, d_x, d_xa, d_sa, d_se, d_y, d_fx, nblk, xa_per_profile,
 * se_full; the same shapes) and writes
 *   d_status     [nprof] uint8           as mwrt_oe_step_device                                    required
 *   d_gain       [nprof][m][n]           gain^T; 0 in a dropped row                                optional
 *   d_ksa        [nprof][m][n]           W = K Sa; 0 in a dropped row                              optional
 *   d_keep       [nprof][m] uint8        1: the row is used                                        optional
 *   d_avk_diag, d_noise_var, d_smooth_var   [nprof][nblk][nlev]                                    optional
 *   d_dfs_block  [nprof][nblk]                                                                     optional
 *   d_nobs       [nprof] int32           m_used                                                    optional
 *   Every output but d_status is optional (NULL: not wanted), but at least one of them must be given.
 *   status 3 (nothing observed): gain 0, W 0, keep 0, avk_diag 0, dfs_block 0, noise_var 0, smooth_var = diag Sa, nobs 0.
 *   status 0 and 2: every floating-point output of the profile NaN, keep 0; nobs as in the step (0, m_used).
 * mwrt_oe_product_device reads what `product` names and writes rows row_begin .. row_begin + row_count - 1 of the n x n
 * result to d_out [nprof][row_count][n]; row_count == 0 with row_begin == 0 means all n rows.
 *   MWRT_OE_PRODUCT_AVK        d_out = gain K        reads d_gain, d_keep, d_k
 *   MWRT_OE_PRODUCT_POST_COV   d_out = Sa - gain W   reads d_gain, d_keep, d_ksa, d_sa
 *   A row of K or W whose d_keep is 0 is never read (a dropped row of K may hold NaN); it contributes nothing.  An element
 *   of the result is the same bit for bit whatever window it is computed in.  A profile whose gain is NaN (status 0, 2)
 *   has keep 0 throughout, so its A is 0 and its S^ is Sa: read d_status before using either.
 * Determinism: a profile's outputs depend on neither its batch-mates nor nprof (fixed summation orders, no atomics), and
 *   the gain does not depend on which optional outputs are asked for.
 * The record starts with its own size: fields at or beyond struct_size (and a field it ends inside) are taken as NULL / 0.
 * Limits: m <= MWRT_OE_MAX_M, nlev <= MWRT_MAX_LEVELS: MWRT_ERR_UNSUPPORTED with the limit in the error text (and for a
 *   product of more than 2^31 - 1 tiles of 64 x 64 in one call).  MWRT_ERR_INVALID_ARGUMENT: a NULL pointer among those the
 *   call reads or must write (gain: the inputs and d_status, and all of the optional outputs at once; product: d_gain,
 *   d_keep, d_out and what its product reads), nblk outside 1 .. 4, reserved or reserved2 != 0, nlev < 1, m < 1,
 *   nprof < 0, struct_size smaller than the fixed part (24 bytes); product alone: an unknown `product`, row_begin < 0,
 *   row_count < 0, a window that runs over n, row_count == 0 with row_begin != 0.
 * Streams as every *_device entry.  The calls never allocate and never synchronise; the gain kernel's dynamic-LDS limit is
 *   raised once per device and size above 64 KiB (m >= 65), so a repeat call of the same size is the launch alone.
 *   (MWRT_VERSION stays 301: additions.) */
#define MWRT_OE_PRODUCT_AVK       0   /* d_out = gain^T K            (reads d_gain, d_keep, d_k)        */
#define MWRT_OE_PRODUCT_POST_COV  1   /* d_out = Sa - gain^T (K Sa)  (reads d_gain, d_keep, d_ksa, d_sa) */
typedef struct mwrt_oe_char {
  uint32_t struct_size;        /* sizeof(mwrt_oe_char) of the caller; fields beyond it are not read */
  int32_t  nblk, xa_per_profile, se_full, reserved;
  const double* d_k[4];
  const double *d_x, *d_xa, *d_sa, *d_se, *d_y, *d_fx;
  uint8_t* d_status;                                   /* gain entry: required                        */
  double *d_gain, *d_ksa;  uint8_t* d_keep;            /* [nprof][m][n], [nprof][m][n], [nprof][m]     */
  double *d_avk_diag, *d_dfs_block, *d_noise_var, *d_smooth_var;  int32_t* d_nobs;
  int32_t product, row_begin, row_count, reserved2;    /* product entry                               */
  double* d_out;                                       /* [nprof][rows][n]                            */
} mwrt_oe_char;
int mwrt_oe_gain_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, void* stream);
int mwrt_oe_product_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_char* s, void* stream);
/* sizeof(mwrt_oe_char) as compiled into the library (binding self-check). */
size_t mwrt_oe_char_size(void);

/* The instrument operator: channel quantities from monochromatic pencil-beam ones.  A radiometer channel
 * integrates over its bandpass and its antenna beam; on a quadrature grid of m_in = nang_q * nf_q (elevation, frequency)
 * nodes that is a fixed sparse linear map onto m_out = nang * nch (elevation, channel) outputs,
 *     y_o = sum_e w[e] TB[col[e]],     K_o[l] = sum_e w[e] K[col[e]][l],     e in [row_ptr[o], row_ptr[o + 1])
 * with the same weights for the brightness temperatures and for every row of every K-matrix block.  The operator is a
 * handle like a model: mwrt_obs_create checks the HOST arrays row_ptr [m_out + 1], col [nnz] and w [nnz] (CSR;
 * nnz = row_ptr[m_out]) and uploads them once, so mwrt_obs_apply_device is the launch alone.
 *   mwrt_obs_create refuses with MWRT_ERR_INVALID_ARGUMENT: a NULL argument, m_in < 1 or m_out < 1, row_ptr[0] != 0, a
 *   row_ptr that decreases, a col outside 0 .. m_in - 1, a weight that is not finite.  Columns need not be sorted and may
 *   repeat within a row and between rows; a row may be empty.
 *   mwrt_obs_destroy(NULL) is MWRT_OK.  A live operator drains the device first (a queued launch may still read it).
 *   mwrt_obs_destroy and mwrt_destroy of the operator's context may come in either order: mwrt_destroy frees the device
 *   copy of every operator still alive on the context and leaves the handles valid for mwrt_obs_destroy alone (apply then
 *   refuses them).
 * mwrt_obs_apply_device, all DEVICE pointers, float64, on `stream` as every *_device entry:
 *   d_tb_in  [nprof][m_in]        -> d_tb_out  [nprof][m_out]           optional, as a pair
 *   d_k_in[b][nprof][m_in][nlev]  -> d_k_out[b][nprof][m_out][nlev]     b < nblk, nblk 0 .. 4
 *   (a Jacobian output [nprof][nang_q][nf_q][nlev] as that entry wrote it; the result is [nprof][nang][nch][nlev] when the
 *   rows are ordered o = a * nch + c).  One launch for the K blocks and one for the TB pair (the same kernel with nlev = 1).
 *   The sum of a row is FMA-accumulated from 0.0 in the stored order of its entries: an element of the result is the same
 *   bit for bit whatever nprof, the blocks and pairs asked for, or the call.  An empty row gives exactly 0.0.  NaN and Inf
 *   propagate through the entries that reference them and through no others (what a dense product with the [m_out][m_in]
 *   matrix would not do); an explicit zero weight on a NaN input gives NaN (IEEE).
 *   Refused with MWRT_ERR_INVALID_ARGUMENT, nothing written: a NULL context, operator or record; an operator of another
 *   context, or one whose context was destroyed; struct_size smaller than the fixed part (12 bytes); nblk outside 0 .. 4;
 *   reserved != 0; one pointer of a pair given without the other; a NULL pointer among the first nblk of d_k_in or
 *   d_k_out; nothing to do (no TB pair and nblk = 0); an output pointer equal to its input; nlev < 1; nprof < 0.
 *   MWRT_ERR_UNSUPPORTED: nlev > MWRT_MAX_LEVELS; more than 2^31 - 1 workgroups in one launch.  nprof = 0 is MWRT_OK.
 *   The record starts with its own size: fields at or beyond struct_size (and a field it ends inside) are taken as NULL.
 *   The call never allocates and never synchronises; it is hipGraph-capturable from the first call.
 *   (MWRT_VERSION stays 301: additions.) */
typedef struct mwrt_obs mwrt_obs;           /* device-resident copy of the CSR map, owned by one context */
typedef struct mwrt_obs_apply {
  uint32_t struct_size;        /* sizeof(mwrt_obs_apply) of the caller; fields beyond it are not read */
  int32_t  nblk, reserved;
  const double* d_tb_in;  double* d_tb_out;            /* [nprof][m_in] -> [nprof][m_out]              */
  const double* d_k_in[4];                             /* [nprof][m_in][nlev]                          */
  double* d_k_out[4];                                  /* [nprof][m_out][nlev]                         */
} mwrt_obs_apply;
int mwrt_obs_create(mwrt_context* ctx, int32_t m_in, int32_t m_out, const int32_t* row_ptr, const int32_t* col,
                    const double* w, mwrt_obs** out);
int mwrt_obs_destroy(mwrt_obs* op);
int mwrt_obs_apply_device(mwrt_context* ctx, const mwrt_obs* op, int64_t nprof, int32_t nlev, const mwrt_obs_apply* rec,
                          void* stream);
/* sizeof(mwrt_obs_apply) as compiled into the library (binding self-check). */
uint32_t mwrt_obs_apply_size(void);

/* The reduced-basis state: x = x_ref + B c with a basis B [n][r] shared by the batch, n = nblk * nlev (state
 * index = block * nlev + level) and r columns (leading EOFs of the prior, coarse layers, one scale factor on a profile
 * shape, ...).  The 1D-Var update in the coefficients c needs K B instead of K, and the optimal-estimation entries take it
 * as they are: d_k[0] = K_c with nblk = 1, nlev = r, the state c, its prior c_a and its covariance [r][r].
 *   mwrt_basis_create checks the HOST array b [nblk * nlev][r] (row-major, column index fastest) and uploads it once.  It
 *   refuses with MWRT_ERR_INVALID_ARGUMENT: a NULL argument, nblk outside 1 .. 4, nlev < 1, r < 1, an entry of b that is
 *   not finite; with MWRT_ERR_UNSUPPORTED: nlev or r > MWRT_MAX_LEVELS.
 *   mwrt_basis_destroy(NULL) is MWRT_OK.  A live basis drains the device first (a queued launch may still read it).
 *   mwrt_basis_destroy and mwrt_destroy of the basis' context may come in either order: mwrt_destroy frees the device copy
 *   of every basis still alive on the context and leaves the handles valid for mwrt_basis_destroy alone (project and expand
 *   then refuse them).
 * mwrt_basis_project_device, all DEVICE pointers, float64, on `stream` as every *_device entry:
 *   d_k_in[b] [nprof][m][nlev], b < nblk of the basis  ->  d_k_out [nprof][m][r],
 *       K_c[p][i][j] = sum over b, l of K_b[p][i][l] * B[b * nlev + l][j]
 *   (a Jacobian output [nprof][nang][nf][nlev] as that entry wrote it, or mwrt_obs_apply_device's).  Every element is one
 *   FMA chain from 0.0 over b = 0 .. nblk - 1 (outer) and l = 0 .. nlev - 1 (ascending): the same bit for bit whatever
 *   nprof, the rows beside it, the other columns of the basis, or the call.  A NaN or Inf in K makes its own output row
 *   [p][i][:] non-finite and reaches no other row (the step's row rule then drops that observation); a row of zeros gives
 *   exactly 0.0.
 * mwrt_basis_expand_device:  d_c [nprof][r], d_x_ref [n] (or [nprof][n] with x_ref_per_profile != 0)  ->  d_x [nprof][n],
 *       x[p][k] = x_ref[k] + sum over j of B[k][j] * c[p][j]
 *   FMA-accumulated onto x_ref[k] for j = 0 .. r - 1 ascending.  A non-finite c[p] makes x[p][:] non-finite and no other.
 * Both refuse with MWRT_ERR_INVALID_ARGUMENT, nothing written: a NULL context, basis or record; a basis of another context,
 *   or one whose context was destroyed; struct_size smaller than the fixed part (8 bytes); reserved or reserved2 != 0;
 *   nprof < 0; project: m < 1, a NULL among the first nblk of d_k_in, a NULL d_k_out, d_k_out equal to one of its inputs;
 *   expand: a NULL d_c, d_x_ref or d_x, d_x equal to d_c or d_x_ref.  MWRT_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups
 *   in one launch.  nprof = 0 is MWRT_OK.
 *   The record starts with its own size: fields at or beyond struct_size (and a field it ends inside) are taken as NULL / 0.
 *   The calls never allocate and never synchronise; they are hipGraph-capturable from the first call.
 *   (MWRT_VERSION stays 301: additions.) */
typedef struct mwrt_basis mwrt_basis;       /* device-resident copy of B, owned by one context */
typedef struct mwrt_basis_apply {
  uint32_t struct_size;        /* sizeof(mwrt_basis_apply) of the caller; fields beyond it are not read */
  int32_t  reserved;
  const double* d_k_in[4];  double* d_k_out;                        /* project */
  const double *d_c, *d_x_ref;  double* d_x;                        /* expand  */
  int32_t  x_ref_per_profile, reserved2;
} mwrt_basis_apply;
int mwrt_basis_create(mwrt_context* ctx, int32_t nblk, int32_t nlev, int32_t r, const double* b, mwrt_basis** out);
int mwrt_basis_destroy(mwrt_basis* basis);
int mwrt_basis_project_device(mwrt_context* ctx, const mwrt_basis* basis, int64_t nprof, int32_t m,
                              const mwrt_basis_apply* rec, void* stream);
int mwrt_basis_expand_device(mwrt_context* ctx, const mwrt_basis* basis, int64_t nprof, const mwrt_basis_apply* rec,
                             void* stream);
/* sizeof(mwrt_basis_apply) as compiled into the library (binding self-check). */
uint32_t mwrt_basis_apply_size(void);

/* Pre-whitening with a per-profile observation-error covariance.  The optimal-estimation entries take one
 * Se for the batch.  With Se_p = L_p L_p^T (Cholesky) on the rows profile p keeps,
 *     K~ = L^-1 K,    y~ = L^-1 y,    F~ = L^-1 F(x)
 * make mwrt_oe_step_device, the Levenberg-Marquardt split, mwrt_oe_cost_device and mwrt_oe_gain_device, called with
 * Se = 1 ([m] ones), compute exactly the x_new, chi2, dfs, post_var, A, S^, budget and cost J of the step with Se_p; only the
 * gain has to be restored, gain = L^-T gain~.  All DEVICE pointers, float64, on `stream` as every *_device entry.
 * mwrt_obs_whiten_device decides, factorises and applies:
 *   in:   d_se [nprof][m] variances, or [nprof][m][m] symmetric (the lower triangle is read) with se_full != 0;
 *         d_y, d_fx [nprof][m];  d_k_in[b] [nprof][m][nlev], b < nblk, nblk 0 .. 4 (a Jacobian output,
 *         mwrt_obs_apply_device's rows, or mwrt_basis_project_device's K B with nlev := r)
 *   out:  d_l [nprof][m (m + 1) / 2], the lower triangle packed by rows, L_ij at i (i + 1) / 2 + j;  d_keep [nprof][m] uint8;
 *         d_status [nprof] uint8;  optional, each on its own: d_y_out, d_fx_out [nprof][m], d_k_out[b] [nprof][m][nlev]
 *   Row rule, that of mwrt_oe_step_device: row i is kept when y_i, fx_i, every K_b[i][:] and its Se entry -- the variance,
 *   or every element of row i of a full Se_p -- are finite.  A dropped row is deleted from Se_p BEFORE the factorisation (a
 *   NaN left inside would reach every later row through L): d_l is the factor of the kept sub-matrix in full indexing, a
 *   dropped row being a row of the identity.  In the outputs a dropped row is NaN in y_out and fx_out, so that the step's
 *   own row rule drops the same rows, and exact 0.0 in the K blocks.
 *   status 1: ok.  2: a pivot fails pivot > 0 (the kept Se_p is not positive definite): d_l and every other floating-point
 *   output of the profile are NaN, keep is 0.  3: no row kept: y_out, fx_out NaN, K rows 0.0, keep 0, L the identity.
 *   Arithmetic, fixed per element: the Cholesky is that of the step's kernels (right-looking, column by column); then per
 *   column v:  acc = v_i;  for j < i ascending: acc = fma(-L_ij, w_j, acc);  w_i = acc / L_ii, where a dropped row takes
 *   part as w_j = 0 with L_ij = 0 (its input is loaded first and selected afterwards: 0 * NaN never gets in).  A profile's
 *   outputs depend on neither its batch-mates, nprof, the column's neighbours nor the outputs asked for.  No atomics.
 *   mode must be 0.
 * mwrt_obs_whiten_apply_device applies a stored d_l and d_keep (inputs here; d_se and d_status are not read) to the vectors
 *   d_y -> d_y_out and d_fx -> d_fx_out (each optional, as a pair) and to the blocks d_k_in[b] -> d_k_out[b], b < nblk:
 *   mode 0: L^-1, as above, bit for bit what mwrt_obs_whiten_device wrote from the same inputs (F(x_trial) of a damped
 *           iteration on the rows of its linearisation; a non-finite value in a kept row stays in that row and reaches the
 *           kept rows after it, so mwrt_oe_cost_device returns +inf and the trial is rejected);
 *   mode 1: L^-T:  i descending, acc = v_i;  for j > i descending: acc = fma(-L_ji, w_j, acc);  w_i = acc / L_ii (the
 *           [nprof][m][n] gain of mwrt_oe_gain_device with nlev := n, so that it is d x^ / d y again).
 *   In both modes a dropped row is exact 0.0 in a block and NaN in a vector, and a profile whose d_l[0] is NaN (status 2)
 *   gets NaN in every output.
 * Both refuse with MWRT_ERR_INVALID_ARGUMENT, nothing written: a NULL context or record; struct_size smaller than the fixed
 *   part (24 bytes); nblk outside 0 .. 4; reserved != 0; an unknown mode; m < 1, nlev < 1, nprof < 0; a NULL among the
 *   required pointers (whiten: d_se, d_y, d_fx, d_l, d_keep, d_status, the first nblk of d_k_in; apply: d_l, d_keep, the
 *   first nblk of d_k_in and d_k_out); apply: one of a vector pair without the other, nothing to do (no vector and
 *   nblk = 0); an output pointer equal to an input.  MWRT_ERR_UNSUPPORTED: m > MWRT_OE_MAX_M, nlev > MWRT_MAX_LEVELS, more
 *   than 2^31 - 1 workgroups in one launch.  nprof = 0 is MWRT_OK.
 *   The record starts with its own size: fields at or beyond struct_size (and a field it ends inside) are taken as NULL.
 *   The calls never allocate and never synchronise; after a first call of the same m they are the launches alone (beyond
 *   m = 120 the kernels' dynamic LDS limit is raised once per device).  Timing: DESIGN.md 4.10.
 *   (MWRT_VERSION stays 301: additions.) */
typedef struct mwrt_obs_whiten {
  uint32_t struct_size;        /* sizeof(mwrt_obs_whiten) of the caller; fields beyond it are not read */
  int32_t  nblk, se_full, mode;
  int64_t  reserved;
  const double *d_se, *d_y, *d_fx;
  const double* d_k_in[4];                             /* [nprof][m][nlev]                             */
  double* d_l;  uint8_t* d_keep;  uint8_t* d_status;   /* out of whiten; d_l, d_keep in of apply       */
  double *d_y_out, *d_fx_out;
  double* d_k_out[4];                                  /* [nprof][m][nlev]                             */
} mwrt_obs_whiten;
int mwrt_obs_whiten_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* rec,
                           void* stream);
int mwrt_obs_whiten_apply_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_obs_whiten* rec,
                                 void* stream);
/* sizeof(mwrt_obs_whiten) as compiled into the library (binding self-check). */
uint32_t mwrt_obs_whiten_size(void);

/* The same step in the n-form (Rodgers 2000, eq. 5.9 and, damped, eq. 5.36 as printed): an n x n system
 * per profile instead of an m x m one, for small states (a reduced basis, a coarse grid) and ANY number of observations:
 *     H = K^T W K,  g = K^T W r,  r = y - F(x),  W = diag(1 / se_i) over the rows kept
 *     C = H + (1 + gamma) Sa^-1 = L L^T,      x+ = x + C^-1 [ g - Sa^-1 (x - xa) ]
 * gamma = 0 gives mwrt_oe_step_device's x+ and C^-1 is the posterior covariance.  Nothing of size m x m exists.
 *   mwrt_oe_nform_prepare_device   the linearisation at x: the row rule, H, g and r^T W r in ONE pass over K
 *   mwrt_oe_nform_solve_device     one (optionally damped) step on a linearisation, and the diagnostics at gamma = 0
 *   mwrt_oe_nform_cost_device      J = sum_kept (y - fx)^2 / se + (x - xa)^T Sa^-1 (x - xa) at a state, on a linearisation's rows
 * One record, mwrt_oe_nform, serves the three.  Layouts are those of mwrt_oe_step / mwrt_oe_lm (all DEVICE pointers,
 * float64 unless stated): d_k[b], b < nblk (1 .. 4), [nprof][m][nlev] -- with a reduced basis the one block K B
 * [nprof][m][r] and nlev = r; d_x the current state; d_xa shared or, with xa_per_profile != 0, per profile; d_y, d_fx
 * [nprof][m]; and
 *   d_sa_inv     [n][n]                  Sa^-1, SYMMETRIC, formed by the caller as for mwrt_oe_cost_device   (solve, cost)
 *   d_se         [m], or [nprof][m] with se_per_profile != 0: VARIANCES ONLY.  A full Se is not taken by this family
 *                                        (whiten first: mwrt_obs_whiten_device, then variances of 1)         (prepare, cost)
 *   d_gamma      [nprof], optional       the damping factor; NULL: gamma = 0                                  (solve)
 *   d_active     [nprof] uint8, optional a profile whose flag is 0 is skipped: NONE of its outputs is touched (all three)
 * The linearisation, written by prepare to caller-owned buffers, read by solve (d_h, d_g, d_rwr, d_lin_status) and by
 * cost (d_keep):
 *   d_keep       [nprof][m] uint8        1: the row is used.  The row rule is that of mwrt_oe_step_device: row i is dropped
 *                                        when y_i, fx_i, any K[i, :] or its variance is not finite
 *   d_nobs       [nprof] int32           m_used
 *   d_h          [nprof][n (n + 1) / 2]  packed lower triangle of H, entry (i, j <= i) at i (i + 1) / 2 + j
 *   d_g          [nprof][n]              K^T W r
 *   d_rwr        [nprof]                 r^T W r
 *   d_lin_status [nprof] uint8           1 ok;  0 x or xa not finite (h, g, rwr NaN, keep 0, nobs 0);  2 a kept row's
 *                                        variance is <= 0 (h, g, rwr NaN; keep and nobs as decided);  3 no usable row
 *                                        (h, g, rwr, keep and nobs 0)
 * Outputs of solve: d_x_new [nprof][nblk][nlev] and d_status [nprof] uint8 required.  Optional, defined at gamma = 0 only
 *   (a call that gives d_gamma and asks for one of them is MWRT_ERR_INVALID_ARGUMENT):
 *   d_chi2     [nprof]              d^T G^-1 d, the m-form step's chi2, formed without a second pass over K as the cost at
 *                                   the linear solution: with s = x+ - x and e = x+ - xa,
 *                                   (r^T W r - 2 s^T g + s^T H s) + e^T Sa^-1 e; its rounding error scales with d^T W d
 *   d_dfs      [nprof]              tr(C^-1 H), summed element by element in a fixed order
 *   d_post_var [nprof][nblk][nlev]  diag C^-1
 *   d_post_cov [nprof][n][n]        C^-1, full and symmetric
 *   status: 1 ok;  0 d_lin_status 0, or x / xa not finite now: outputs NaN;  2 d_lin_status 2, gamma negative or not
 *   finite, or a Cholesky pivot fails pivot > 0: outputs NaN;  3 d_lin_status 3: x_new = xa + gamma / (1 + gamma) (x - xa)
 *   (xa exactly at gamma = 0), chi2 and dfs 0, post_var and post_cov from the inverse of Sa^-1 as computed (NaN when that
 *   factorisation fails).  x_new does not depend on which optional outputs are asked for.
 * Outputs of cost: d_cost [nprof] required; d_cost_obs, d_cost_prior [nprof] and d_status optional.  A non-finite x or
 *   xa, or y or fx in a kept row, gives +inf in all three with status 1 (a trial to reject, as in mwrt_oe_cost_device); a
 *   kept row's variance <= 0 gives NaN in all three and status 2.
 * Determinism: a profile's outputs depend on neither its batch-mates nor nprof (one workgroup per profile, every sum in
 *   one fixed order, no atomics).  No workspace: the calls never allocate and never synchronise; a launch above 64 KiB of
 *   dynamic LDS (solve from n = 122 on) raises that kernel's limit once per device and size, so the entries are
 *   hipGraph-capturable after one warm-up call.
 * Limits: n = nblk * nlev <= MWRT_OE_NFORM_MAX_N (the packed triangle of C lives in LDS): beyond it MWRT_ERR_UNSUPPORTED
 *   with the limit in the text.  m >= 1 and otherwise unbounded: MWRT_OE_MAX_M does not apply.  MWRT_ERR_INVALID_ARGUMENT,
 *   checked in this order: struct_size smaller than the fixed part (24 bytes); nprof < 0, nlev < 1 or m < 1; nblk outside
 *   1 .. 4; reserved != 0; a NULL pointer among those the call reads or must write (prepare: d_k, d_x, d_xa, d_se, d_y,
 *   d_fx and the linearisation; solve: d_x, d_xa, d_sa_inv, d_h, d_g, d_rwr, d_lin_status, d_x_new, d_status; cost: d_x,
 *   d_xa, d_sa_inv, d_se, d_y, d_fx, d_keep, d_cost); d_gamma with a gamma = 0-only output.  nprof = 0 is MWRT_OK and
 *   launches nothing.  The record starts with its own size: fields at or beyond struct_size (and a field it ends inside)
 *   are taken as NULL.  Measured on an MI355X (profiles/nform_errors.json, profiles/nform_time.json): x_new
 *   within 1.1e-12 of the reference in units of max |x+ - xa| per block; at 1000 profiles x 98 observations and r = 32,
 *   prepare 0.049 ms and solve 0.045 ms against 0.83 ms of mwrt_oe_step_device on the same K B.
 *   (MWRT_VERSION stays 301: additions.) */
#define MWRT_OE_NFORM_MAX_N 128
typedef struct mwrt_oe_nform {
  uint32_t struct_size;        /* sizeof(mwrt_oe_nform) of the caller; fields beyond it are not read */
  int32_t  nblk, xa_per_profile, se_per_profile, reserved;
  const double* d_k[4];
  const double *d_x, *d_xa, *d_sa_inv, *d_se, *d_y, *d_fx;
  const double* d_gamma;
  const uint8_t* d_active;
  double *d_h, *d_g, *d_rwr;  uint8_t* d_keep;  int32_t* d_nobs;  uint8_t* d_lin_status;   /* the linearisation */
  double* d_x_new;  uint8_t* d_status;                 /* required outputs of solve; d_status optional in cost */
  double *d_chi2, *d_dfs, *d_post_var, *d_post_cov;    /* optional outputs of solve, gamma = 0 only */
  double *d_cost, *d_cost_obs, *d_cost_prior;          /* outputs of cost */
} mwrt_oe_nform;
int mwrt_oe_nform_prepare_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream);
int mwrt_oe_nform_solve_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream);
int mwrt_oe_nform_cost_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform* s, void* stream);
/* sizeof(mwrt_oe_nform) as compiled into the library (binding self-check). */
size_t mwrt_oe_nform_size(void);

/* The characterisation of the n-form step (Rodgers 2000, ch. 3): what mwrt_oe_gain_device and
 * mwrt_oe_product_device give the m-form, from the n x n objects a linearisation already holds and one pass over K.  At
 * gamma = 0, with H = K^T W K as mwrt_oe_nform_prepare_device wrote it, C = H + Sa^-1 = L L^T and S^ = C^-1:
 *     A      = S^ H                        [n][n]  averaging kernel (= I - S^ Sa^-1)
 *     gain^T = W K S^, row i = S^ k_i / se_i [m][n]  contribution functions d x^ / d y_i; 0 in a dropped row
 *     noise  = diag(S^ H S^) = diag(A S^)  [n]     = diag(gain Se gain^T)
 *     smooth = diag S^ - noise             [n]     = diag((A - I) Sa (A - I)^T)
 *     avk_diag = diag A;  dfs_block[b] = sum of avk_diag over block b;  their sum is tr(C^-1 H), the solve's dfs
 *   mwrt_oe_nform_char_device   S^, A (a row window), avk_diag, dfs_block, noise and smooth from a linearisation
 *   mwrt_oe_nform_gain_device   the gain from K, the row rule, the variances and S^
 * These are the diagnostics of the UNDAMPED step: there is no d_gamma, and neither entry reads x, xa, y or fx.  One record,
 * mwrt_oe_nform_char, serves both (all DEVICE pointers, float64 unless stated; n = nblk * nlev, state index = block *
 * nlev + level):
 *   d_k[b]       [nprof][m][nlev], b < nblk   the rows prepare saw                                           (gain)
 *   d_sa_inv     [n][n]                  Sa^-1, SYMMETRIC, as for mwrt_oe_nform_solve_device                (char)
 *   d_se         [m], or [nprof][m] with se_per_profile != 0: VARIANCES, as prepare saw them                (gain)
 *   d_h          [nprof][n (n + 1) / 2]  packed H as prepare wrote it                                       (char)
 *   d_lin_status [nprof] uint8           as prepare wrote it                                                (char)
 *   d_keep       [nprof][m] uint8        as prepare wrote it                                                (gain)
 *   d_active     [nprof] uint8, optional a profile whose flag is 0 is skipped: NONE of its outputs is touched (both)
 * Outputs of char: d_status [nprof] uint8 required; each of the others optional, but at least one must be given:
 *   d_post_cov   [nprof][n][n]           S^, full and symmetric
 *   d_avk        [nprof][rows][n]        rows row_begin .. row_begin + row_count - 1 of A, with the window of
 *                                        mwrt_oe_product_device: row_count == 0 with row_begin == 0 means all n rows
 *   d_avk_diag, d_noise_var, d_smooth_var [nprof][nblk][nlev];   d_dfs_block [nprof][nblk]
 *   status: 1 ok;  0 d_lin_status is 0: every floating-point output of the profile is NaN;  2 d_lin_status is 2 (or
 *   anything but 0, 1, 3), or a Cholesky pivot fails pivot > 0: every floating-point output is NaN;  3 d_lin_status is 3:
 *   A, avk_diag, dfs_block and noise_var are exactly 0, S^ is the inverse of Sa^-1 as computed and smooth_var its diagonal
 *   (both NaN when that factorisation fails; status stays 3, as in the solve).
 *   Only the rows of A a call needs are formed (the window; all of them for noise_var or smooth_var), and S^ leaves the
 *   workgroup only when d_post_cov is given: d_avk_diag and d_dfs_block alone cost n^2 per profile behind the inverse.
 * gain: inputs d_k, d_se, d_keep, d_post_cov and d_status -- those mwrt_oe_nform_char_device wrote, or the d_post_cov and
 *   d_status mwrt_oe_nform_solve_device wrote at gamma = 0; output d_gain [nprof][m][n], required.  A row whose keep is 0
 *   is never used and gives exact 0.0 (it may hold NaN: the select comes after the load); a profile whose d_status is 0
 *   or 2 gets NaN throughout, one whose d_status is 3 gets 0.0 throughout.  A kept row with a variance <= 0 cannot occur
 *   (its d_lin_status is 2, so its d_status is 2).  The row window is not read.
 * Determinism: a profile's outputs depend on neither its batch-mates nor nprof, nor on which optional outputs are asked
 *   for.  An element of A is the same bit for bit in whatever row window it is computed, an element of the gain in whatever
 *   row tile it falls: every sum is one fixed-order chain of fused multiply-adds (the sums over lanes and blocks a fixed
 *   tree).  No atomics, no matrix instructions.  No workspace: the calls never allocate and never synchronise; a char launch
 *   above 64 KiB of dynamic LDS (from n = 89 on) raises the kernel's limit once per device and size, so the entries are
 *   hipGraph-capturable after one warm-up call.
 * Refused, checked in this order, nothing written.  MWRT_ERR_INVALID_ARGUMENT: a NULL context or record; struct_size
 *   smaller than the fixed part (24 bytes); nprof < 0, nlev < 1 or m < 1; nblk outside 1 .. 4; reserved != 0; char:
 *   row_begin < 0, row_count < 0, a window that runs over n, row_count == 0 with row_begin != 0; a NULL pointer among those
 *   the call requires (char: d_sa_inv, d_h, d_lin_status, d_status; gain: the first nblk of d_k, d_se, d_keep, d_post_cov,
 *   d_status, d_gain); char with no output beside d_status; an output pointer equal to an input of the call.
 *   MWRT_ERR_UNSUPPORTED: n = nblk * nlev > MWRT_OE_NFORM_MAX_N, with the limit in the text; more than 2^31 - 1 workgroups
 *   in one launch (char: one per profile; gain: nprof * ceil(m / 128) row tiles).  nprof = 0 is MWRT_OK and launches
 *   nothing.  m is not bounded.  The record starts with its own size: fields at or beyond struct_size (and a field it ends
 *   inside) are taken as NULL / 0.  Accuracy and timing: DESIGN.md 4.11.1.
 *   (MWRT_VERSION stays 301: additions.) */
typedef struct mwrt_oe_nform_char {
  uint32_t struct_size;        /* sizeof(mwrt_oe_nform_char) of the caller; fields beyond it are not read */
  int32_t  nblk, se_per_profile, row_begin, row_count, reserved;
  const double* d_k[4];
  const double *d_sa_inv, *d_se, *d_h;
  const uint8_t *d_lin_status, *d_keep, *d_active;
  uint8_t* d_status;                                   /* out of char, in of gain */
  double* d_post_cov;                                  /* out of char (optional), in of gain */
  double *d_avk, *d_avk_diag, *d_noise_var, *d_smooth_var, *d_dfs_block;   /* optional outputs of char */
  double* d_gain;                                      /* output of gain */
} mwrt_oe_nform_char;
int mwrt_oe_nform_char_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s, void* stream);
int mwrt_oe_nform_gain_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_nform_char* s, void* stream);
/* sizeof(mwrt_oe_nform_char) as compiled into the library (binding self-check). */
size_t mwrt_oe_nform_char_size(void);

/* Observation selection by information content (Rodgers 2000, section 2.5 and ch. 3; the sequential
 * channel selection of Rabier et al. 2002): which observations of a scan carry the information.  Per profile, with the
 * rows k_i [n] of [K0 | K1 | ...] (n = nblk * nlev), the variances se_i, a start covariance S0 [n][n] (Sa, the sa_c of a
 * basis, or the posterior of an earlier selection) and a candidate set:
 *     q_i = k_i^T S0 k_i / se_i                         the SNR^2 of observation i in the metric of the current posterior
 *   round t = 0 .. nsel - 1:
 *     j = argmax of q_i over the unchosen candidates; ties go to the LOWEST index; stop when the best q is not > 0
 *     v = S k_j;  d = se_j + k_j^T v;  order[t] = j;  q_pick[t] = q_j;  rank[j] = t
 *     dfs_gain[t] = v^T Sa^-1 v / d                     only when d_sa_inv and d_dfs_gain are given
 *     S <- S - v v^T / d                                the posterior after assimilating j
 *     q_i <- max(0, q_i - k_i^T v squared / (d se_i))   for every unchosen candidate, one pass over K
 * The largest q is the largest entropy reduction log2(1 + q) / 2; the bits are formed by the caller from q_pick.  The
 * incremental form of q is the specified one (m n per round instead of m n^2); by Cauchy-Schwarz in the metric of S the
 * term taken off never exceeds q_i.  Row i is a candidate when every element of k_i and se_i is finite, its d_keep flag is
 * 1 and its d_candidate flag is 1 (an absent flag array counts as all 1).  The select comes after the load: a row that is
 * no candidate may hold NaN.  The record (all DEVICE pointers, float64 unless stated):
 *   d_k[b]       [nprof][m][nlev], b < nblk   as for mwrt_oe_nform
 *   d_s0         [n][n], or [nprof][n][n] with s0_per_profile != 0: SYMMETRIC (the lower triangle is the one used)
 *   d_se         [m], or [nprof][m] with se_per_profile != 0: VARIANCES
 *   d_sa_inv     [n][n], optional        Sa^-1, SYMMETRIC; read only together with d_dfs_gain
 *   d_keep       [nprof][m] uint8, optional;   d_candidate [m] uint8, optional;   d_active [nprof] uint8, optional: a
 *                profile whose flag is 0 is skipped and NONE of its outputs is touched
 * Outputs, required: d_order [nprof][nsel] int32 and d_q_pick [nprof][nsel] (unused slots, when fewer than nsel rows are
 *   picked: -1 and 0.0); d_rank [nprof][m] int32 (-1 for a row not chosen); d_q [nprof][m], also the kernel's work vector:
 *   at the end what each unchosen candidate would still add, its q_pick for a chosen row, exact 0.0 for a row that is no
 *   candidate; d_count [nprof] int32, the picks made; d_status [nprof] uint8.  Optional: d_dfs_gain [nprof][nsel] (unused
 *   slots 0.0), d_post_cov [nprof][n][n] the last S, full and symmetric, d_post_var [nprof][nblk][nlev] its diagonal.
 *   status: 1 ok;  0 S0 (or Sa^-1 when read) is not finite: every floating-point output of the profile is NaN, order and
 *   rank are -1, count is 0;  2 a candidate's variance is <= 0, or some d is not > 0 or not finite: the same outputs as 0;
 *   3 no candidate: count is 0, order is -1, post_cov is S0 exactly and post_var its diagonal.
 * Determinism: a profile's outputs depend on neither its batch-mates nor nprof, nor on which optional outputs are asked
 *   for.  Every sum has one fixed order; no atomics, no matrix instructions.  Two bit-identical rows with
 *   bit-identical variances have bit-identical q in every round, whatever their indices, which is what makes the
 *   lowest-index rule observable.  No workspace: the call never allocates and never synchronises; a launch above 64 KiB of
 *   dynamic LDS (from n = 125 on) raises the kernel's limit once per device and size, so the entry is hipGraph-capturable
 *   after one warm-up call.  K is read nsel + 1 times.
 * Refused, checked in this order, nothing written.  MWRT_ERR_INVALID_ARGUMENT: a NULL context or record; struct_size
 *   smaller than the fixed part (24 bytes); nprof < 0, nlev < 1 or m < 1; nblk outside 1 .. 4; reserved != 0; nsel < 1 or
 *   nsel > m; a NULL pointer among those required (the first nblk of d_k, d_s0, d_se, d_order, d_q_pick, d_rank, d_q,
 *   d_count, d_status); d_dfs_gain without d_sa_inv; an output pointer equal to an input.  MWRT_ERR_UNSUPPORTED: n = nblk *
 *   nlev > MWRT_OE_NFORM_MAX_N, with the limit in the text; more than 2^31 - 1 profiles.  nprof = 0 is MWRT_OK and launches
 *   nothing.  m is not bounded.  The record starts with its own size: fields at or beyond struct_size (and a field it ends
 *   inside) are taken as NULL / 0.  Accuracy and timing: DESIGN.md 4.12.
 *   (MWRT_VERSION stays 301: additions.) */
typedef struct mwrt_oe_select {
  uint32_t struct_size;        /* sizeof(mwrt_oe_select) of the caller; fields beyond it are not read */
  int32_t  nblk, se_per_profile, s0_per_profile, nsel, reserved;
  const double* d_k[4];
  const double *d_s0, *d_se, *d_sa_inv;
  const uint8_t *d_keep, *d_candidate, *d_active;
  int32_t* d_order;  double* d_q_pick;                 /* [nprof][nsel], required */
  int32_t* d_rank;   double* d_q;                      /* [nprof][m], required */
  int32_t* d_count;  uint8_t* d_status;                /* [nprof], required */
  double *d_dfs_gain, *d_post_cov, *d_post_var;        /* optional */
} mwrt_oe_select;
int mwrt_oe_select_device(mwrt_context* ctx, int64_t nprof, int32_t nlev, int32_t m, const mwrt_oe_select* s, void* stream);
/* sizeof(mwrt_oe_select) as compiled into the library (binding self-check). */
size_t mwrt_oe_select_size(void);

/* The spectroscopic-parameter Jacobian: d TB / d b for entries b of the model's tables -- what the
 * forward-model part K_b S_b K_b^T of an observation-error covariance is built from (Rodgers 2000, section 3.2.2).  The
 * operator is mwrt_tb_jacobian_batch_device's: clear sky, plane-parallel, every line at every frequency; there is no
 * options argument (cloud, ray tracing and ozone are not built).  A parameter is a (field, line) pair:
 *   scalar fields (line must be 0)   MWRT_PAR_H2O_CF, _H2O_CS, _H2O_XCF, _H2O_XCS (the water-vapour continuum),
 *                                    _O2_X (T exponent of the O2 widths), _O2_WB300 (non-resonant width), _N2_L
 *   H2O per line (0 .. n_h2o - 1)    _H2O_S1, _H2O_B2, _H2O_W0, _H2O_X, _H2O_W0S, _H2O_XS, _H2O_SH, _H2O_SHS
 *   O2 per line  (0 .. n_o2 - 1)     _O2_S300, _O2_BE, _O2_W300, _O2_Y0, _O2_Y1, _O2_G0, _O2_G1, _O2_DNU0, _O2_DNU1
 * each named after the mwrt_model_desc field it differentiates.  line = MWRT_PAR_ALL_LINES on a per-line field asks for
 * the derivative with respect to a common factor s that multiplies that field of EVERY line, at s = 1: the sum over
 * lines k of b_k * d TB / d b_k.  The line centres, the speed-dependent-only fields (w2, d2, ...) and the remaining
 * scalars are not offered.
 *   params     HOST array [npar] (like frq_ghz: a content-keyed device copy is made on first use)
 *   d_tb       [nprof][nang][nf], optional (NULL: not wanted): the TBs of mwrt_tb_jacobian_batch_device, computed by the
 *              same statements from the same absorption arrays (equal to 1e-8 K is what is promised)
 *   d_dtb_db   [nprof][nang][nf][npar] float64, PARAMETER fastest: [nprof][m][npar] with m = nang * nf, so it goes through
 *              mwrt_obs_apply_device with nlev := npar, and into a batched K_b S_b K_b^T, without a copy.  ABSOLUTE
 *              derivatives: K per unit of the table entry as mwrt_model_desc stores it
 *   d_valid    [nprof] as the K-matrix entry
 * Derivative conventions: those of the K-matrix rows, the derivative of the branch the forward takes --
 *   zero slope where max(o2abs, 0) clamps; the 750-GHz cutoff and the speed-dependent switch followed as taken (the
 *   switch's own bound 10 w0 moves with W0, X, W0S, XS: still the branch taken); the layer rule's close-level and zero-end
 *   partials; inside a line's speed-dependent window W0, X, W0S, XS, SH, SHS act through A = w0 - 1.5 w2 + i (d1 + 1.5 delta2).
 *   A parameter the model's modes do not read gives columns of exact 0.0 in every valid row: SH, SHS under
 *   h2o_shift_mode == 0; G0, G1, DNU0, DNU1 under first-order mixing (o2_mix_mode == 0).
 * NaN, valid, streams and capture as mwrt_tb_jacobian_batch_device: a NaN in z / p / T / rh -> valid 0 and NaN in every row
 *   of the profile (d_tb too); a negative absorption coefficient -> valid 2, rows NaN; a NaN elevation blanks only its own
 *   rows; a NaN frequency is MWRT_ERR_INVALID_ARGUMENT; nprof = 0 is MWRT_OK.
 * Refused with MWRT_ERR_INVALID_ARGUMENT, nothing written: a NULL required pointer; npar < 1 or > MWRT_MAX_PARAMS; an
 *   unknown field id; a line outside its table (and not MWRT_PAR_ALL_LINES); line != 0 on a scalar field.
 * Determinism: no floating-point atomics; the sum over levels has a fixed order (lanes of a wave by a shuffle tree, waves in
 *   index order).  A column is the same bit for bit whatever nprof, on a repeat call, and whichever other parameters are
 *   requested beside it and in whatever order (parameters are processed in groups that bound the workspace; a column's
 *   arithmetic does not see its group).
 * Workspace: the K-matrix entry's own (k_absorb_tl fills it: 48 B per (profile, frequency, level); the parameter kernels
 *   read awet, adry and the flags from it) and, for d alpha / d b, 8 B per (profile, frequency, level) and parameter of a
 *   group -- a group being as many parameters as fit 1 GiB, at least one.  Both are owned by the context and only grown
 *   behind a drain.  After one warm-up call with the same shapes, frequencies and parameter list the call neither allocates
 *   nor synchronises (hipGraph-capturable).  nprof * nf * ceil(nlev / 64) > 2^31 - 1 is MWRT_ERR_UNSUPPORTED.
 * Cost: a per-line parameter costs one line's term per (level, frequency); _O2_X and MWRT_PAR_ALL_LINES sum over every line
 *   of their species.  Timing: DESIGN.md 4.8.  (MWRT_VERSION stays 301: additions.) */
#define MWRT_MAX_PARAMS 256
#define MWRT_PAR_ALL_LINES (-1)
#define MWRT_PAR_H2O_CF    0
#define MWRT_PAR_H2O_CS    1
#define MWRT_PAR_H2O_XCF   2
#define MWRT_PAR_H2O_XCS   3
#define MWRT_PAR_O2_X      4
#define MWRT_PAR_O2_WB300  5
#define MWRT_PAR_N2_L      6
#define MWRT_PAR_H2O_S1    7
#define MWRT_PAR_H2O_B2    8
#define MWRT_PAR_H2O_W0    9
#define MWRT_PAR_H2O_X     10
#define MWRT_PAR_H2O_W0S   11
#define MWRT_PAR_H2O_XS    12
#define MWRT_PAR_H2O_SH    13
#define MWRT_PAR_H2O_SHS   14
#define MWRT_PAR_O2_S300   15
#define MWRT_PAR_O2_BE     16
#define MWRT_PAR_O2_W300   17
#define MWRT_PAR_O2_Y0     18
#define MWRT_PAR_O2_Y1     19
#define MWRT_PAR_O2_G0     20
#define MWRT_PAR_O2_G1     21
#define MWRT_PAR_O2_DNU0   22
#define MWRT_PAR_O2_DNU1   23
#define MWRT_PAR_NFIELDS   24
typedef struct mwrt_param { int32_t field; int32_t line; } mwrt_param;
int mwrt_tb_param_jacobian_batch_device(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                        const double* d_z_km, const double* d_p_hpa, const double* d_t_k,
                                        const double* d_rh_frac,
                                        int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                        int32_t npar, const mwrt_param* params,
                                        double* d_tb, double* d_dtb_db, uint8_t* d_valid, void* stream);
/* The same on HOST buffers, synchronous: the arrays are staged through a device buffer of the call's own (freed on every
 * return path) and the device entry is called on the context's stream; the results are its bits.  tb may be NULL. */
int mwrt_tb_param_jacobian_batch(mwrt_context* ctx, const mwrt_model* model, int64_t nprof, int32_t nlev,
                                 const double* z_km, const double* p_hpa, const double* t_k, const double* rh_frac,
                                 int32_t nf, const double* frq_ghz, int32_t nang, const double* elev_deg,
                                 int32_t npar, const mwrt_param* params,
                                 double* tb, double* dtb_db, uint8_t* valid);

/* Diagnostic: evaluates the kernels' own exp / log / division helpers (fexp, flog, fdiv, fdiv1) on
 * host arrays x[n], y_pos[n] (y > 0), so their accuracy can be checked against libm. */
int mwrt_selftest_math(mwrt_context* ctx, int32_t n, const double* x, const double* y_pos,
                       double* exp_x, double* log_y, double* x_div_y, double* x_div1_y);

/* Diagnostic: one of the kernels' other arithmetic helpers on host arrays of n doubles, so each can be held to a
 * high-precision reference on its own arguments.  `helper` selects it (MWRT_HELPER_*; the table says what in0..in3 and
 * out0..out3 mean; arrays a helper does not use may be NULL: unused inputs read as 0, unused outputs are not written);
 * flag[n] (required) receives the helper's `neg` flag, 0 elsewhere.  The kernel runs with `block` threads per workgroup
 * (a multiple of 64 in 64..1024), one thread per element (LAYER_VALUE4: one thread per four consecutive elements, n a
 * multiple of 4); threads past n leave before the helper is called, so the last wave runs its votes with inactive
 * lanes.  The collectives (BLOCK_SUM .. ROW16_MAX) run one workgroup per `block` elements with every thread in the
 * call, those past n holding 0.  An unknown helper, n < 0 or a bad `block` returns MWRT_ERR_INVALID_ARGUMENT; n = 0 is
 * not an error.
 *   FEXP_SMALL, FTANH_HALF_SMALL   in0 = x: out0 = f(x), out1 = f(x, loop_invariant_vgpr(c0))
 *   FEXP_TINY, FTANH_HALF_TINY, TWO_ATANH_TAIL, FSQRT   in0: out0
 *   CRECIP, CSQRT_PRINCIPAL        (in0, in1) = (re, im): (out0, out1)
 *   CMUL_CDIV                      a = (in0, in1), b = (in2, in3): a b in (out0, out1), a / b in (out2, out3)
 *   DCERROR_UPPER                  in0 = x, in1 = y: (out0, out1)
 *   HUI_W_DW                       zh = (in0, in1): w in (out0, out1), dw in (out2, out3)
 *   PLANCK_B                       in0 = x, in1 = 1/x: out0
 *   LAYER_VALUE_ZF1 / _ZF0         in0 = x1, in1 = x0, in2 != 0 = live: out0, flag = neg   (layer_value<true / false>)
 *   LAYER_VALUE4                   in0 = x1, in1 = x0, in2 != 0 = live (read at the thread's first element): out0, flag
 *   LAYER_VALUE_TL_ZF1 / _ZF0      in0 = x1, in1 = x0: out0 = value, out1 = d/dx1, out2 = d/dx0, flag = neg
 *   DIV_SMALL                      in0 = n, in1 = d (integers held in doubles; the magic number is magic_of(d)): out0
 *   BLOCK_SUM, BLOCK_SUFFIX_EXCL   in0: out0;   BLOCK_SCAN   in0: out0 = inclusive prefix, out1 = total
 *   ROW16_MAX                      in0 (rounded to float): out0
 *   WAVE_VOTES                     p = in0 != 0, q = in1 != 0: out0 = wave_all(p), out1 = wave_any(p),
 *                                  out2 = wave_all_of(p, q), as 0 / 1 */
enum {
  MWRT_HELPER_FEXP_SMALL = 0, MWRT_HELPER_FEXP_TINY = 1, MWRT_HELPER_FTANH_HALF_SMALL = 2, MWRT_HELPER_FTANH_HALF_TINY = 3,
  MWRT_HELPER_TWO_ATANH_TAIL = 4, MWRT_HELPER_FSQRT = 5, MWRT_HELPER_CRECIP = 6, MWRT_HELPER_CMUL_CDIV = 7,
  MWRT_HELPER_CSQRT_PRINCIPAL = 8, MWRT_HELPER_DCERROR_UPPER = 9, MWRT_HELPER_HUI_W_DW = 10, MWRT_HELPER_PLANCK_B = 11,
  MWRT_HELPER_LAYER_VALUE_ZF1 = 12, MWRT_HELPER_LAYER_VALUE_ZF0 = 13, MWRT_HELPER_LAYER_VALUE4 = 14,
  MWRT_HELPER_LAYER_VALUE_TL_ZF1 = 15, MWRT_HELPER_LAYER_VALUE_TL_ZF0 = 16, MWRT_HELPER_DIV_SMALL = 17,
  MWRT_HELPER_BLOCK_SUM = 18, MWRT_HELPER_BLOCK_SCAN = 19, MWRT_HELPER_BLOCK_SUFFIX_EXCL = 20, MWRT_HELPER_ROW16_MAX = 21,
  MWRT_HELPER_WAVE_VOTES = 22, MWRT_HELPER_COUNT = 23
};
int mwrt_selftest_helpers(mwrt_context* ctx, int32_t helper, int32_t n, int32_t block,
                          const double* in0, const double* in1, const double* in2, const double* in3,
                          double* out0, double* out1, double* out2, double* out3, uint8_t* flag);

/* Block until everything queued on the context's stream (or `stream`) has finished. */
int mwrt_synchronize(mwrt_context* ctx, void* stream);

/* Kernel timing with HIP events: mwrt_set_timing(ctx, 1) brackets every kernel launch with a
 * hipEvent pair recorded on the launch stream (ring of 512 pairs, no host synchronisation).
 * mwrt_timing_collect sums the device time of the launches since the last collect/enable and
 * returns how many there were; mwrt_last_kernel_ms reads the most recent one. */
int mwrt_set_timing(mwrt_context* ctx, int enabled);
int mwrt_timing_collect(mwrt_context* ctx, double* total_ms, int32_t* launches);
int mwrt_last_kernel_ms(mwrt_context* ctx, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* MWRT_H */
