"""Device time of the pre-whitening with a per-profile Se (mwrt_obs_whiten_device / mwrt_obs_whiten_apply_device, DESIGN
4.10), one process, one stream, HIP events, at the design shape: 1000 profiles x 180 levels x 2 blocks (T, rh) x 98
observations (14 channels x 7 elevations), K from the device K-matrix call on the synthetic profiles, a full Se_p
[1000][98][98], two observations in a hundred missing; and at r = 32 coefficients of the leading eigenvectors of the prior.

  whiten_full / torch_whiten_full    the combined call on both K blocks, y and F | torch on the same buffers:
                                     linalg.cholesky of the masked Se_p and one solve_triangular per block and vector pair
                                     (in chunks of profiles where hipBLAS refuses the whole batch; the chunk is recorded)
  whiten_r32 / torch_whiten_r32      the same on the one block K B [nprof][98][32]
  apply_vec / torch_apply_vec        the stored factor on one vector (F(x_trial) of a damped iteration)
  ungain_full / torch_ungain_full    L^-T on a gain [nprof][98][360];  ungain_r32 / torch_ungain_r32 on [nprof][98][32]
  iter_full / iter_full_se           one full-state iteration (K-matrix call + step) without and with the whitening
  iter_r32 / iter_r32_se             one reduced iteration (K-matrix call + projection + step) without and with it

All paths are run alternately, repetition by repetition, each between one pair of HIP events on the current stream; the
short ones bracket ``--inner`` back-to-back calls.  The file also holds the bytes the whitening pass must move (K in and K
out), the resulting GB/s and its share of the 6.29 TB/s a float4 copy reaches on an MI355X (the figure
tools/obs_apply_time.py uses), and the FMA rate of the substitutions.
Usage: python tools/whiten_time.py [--reps N] [--inner N] [--nprof N] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr
from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis

HBM_MEASURED_TB_S = 6.29
RANK = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    nprof, nlev, frq, ang = a.nprof, pr.N_LEVELS, pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
    nf, nang = frq.size, ang.size
    m, nblk, r = nf * nang, 2, RANK
    n = nblk * nlev
    f64, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.uint8, device="cuda")
    P = pr.synthetic_profiles(nprof, 2)
    z, p, t, rh = (torch.tensor(P[k], **f64) for k in ("z", "p", "t", "rh"))
    tb = torch.empty((nprof, nang, nf), **f64)
    k_t, k_h = (torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(2))
    valid = torch.empty(nprof, **u8)
    variables = nat.JacVariables.of(humidity="rh")
    cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

    def k_matrix():
        ctx.tb_jacobian_batch_vars_device("R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang,
                                          tb.data_ptr(), k_t.data_ptr(), k_h.data_ptr(), valid.data_ptr(), variables=variables,
                                          stream=cur())

    k_matrix()
    torch.cuda.synchronize()
    rng = np.random.default_rng(2010)
    lev = np.arange(nlev)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / (nlev / 6.0))
    sa_h = np.zeros((n, n))
    sa_h[:nlev, :nlev] = 2.0 ** 2 * corr
    sa_h[nlev:, nlev:] = 0.1 ** 2 * corr
    sa_h[:nlev, nlev:] = 0.3 * 2.0 * 0.1 * corr
    sa_h[nlev:, :nlev] = sa_h[:nlev, nlev:].T
    sa, se, ones = torch.tensor(sa_h, **f64), torch.full((m,), 0.25, **f64), torch.ones(m, **f64)
    j = torch.tensor(rng.standard_normal((nprof, m, 6)) * 0.25, **f64)
    se_p = (0.25 * (1.0 + torch.rand(nprof, **f64)))[:, None, None] * torch.eye(m, **f64)[None] + j @ j.transpose(1, 2)
    se_p = se_p.contiguous()
    x = torch.stack([t, rh], dim=1).contiguous()
    xa = (x + torch.tensor(rng.standard_normal((nprof, nblk, nlev)) * np.array([0.5, 0.02])[None, :, None], **f64)).contiguous()
    fx = tb.reshape(nprof, m)
    y = fx + torch.tensor(rng.standard_normal((nprof, m)) * 0.5, **f64)
    y[torch.tensor(rng.random((nprof, m)) < 0.02, device="cuda")] = float("nan")
    chi2, dfs = torch.empty(nprof, **f64), torch.empty(nprof, **f64)
    nobs = torch.empty(nprof, dtype=torch.int32, device="cuda")
    status, wstatus = torch.empty(nprof, **u8), torch.empty(nprof, **u8)
    x_new, post_var = torch.empty_like(x), torch.empty_like(x)
    lpk, keep = torch.empty((nprof, m * (m + 1) // 2), **f64), torch.empty((nprof, m), **u8)
    kw_t, kw_h, y_w, fx_w, v_w = torch.empty_like(k_t), torch.empty_like(k_h), torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
    sb = StateBasis.from_covariance(torch.tensor(sa_h), r)
    _, handle = sb.native_handle(nblk, 0)
    sa_c = sb.sa_c.to("cuda").contiguous()
    k_c, kw_c = torch.empty((nprof, m, r), **f64), torch.empty((nprof, m, r), **f64)
    c, c_a, c_new, pv = torch.zeros((nprof, 1, r), **f64), torch.zeros((1, r), **f64), torch.empty((nprof, 1, r), **f64), torch.empty((nprof, 1, r), **f64)
    gain_full, gain_r = torch.randn((nprof, m, n), **f64), torch.randn((nprof, m, r), **f64)
    ug_full, ug_r = torch.empty_like(gain_full), torch.empty_like(gain_r)
    held = {}

    chunk = {"profiles": nprof}

    def tri_solve(tri, rhs, upper):
        """torch.linalg.solve_triangular over the batch; where hipBLAS cannot allocate its workspace for the whole batch, in
        the largest chunks of profiles it accepts (found once, kept, and written to the file)."""
        while True:
            step = chunk["profiles"]
            try:
                return torch.cat([torch.linalg.solve_triangular(tri[i:i + step], rhs[i:i + step], upper=upper)
                                  for i in range(0, nprof, step)])
            except RuntimeError:
                if step <= 1:
                    raise
                chunk["profiles"] = max(1, step // 2)

    def project():
        ctx.basis_project_device(handle, nprof, m, [k_t.data_ptr(), k_h.data_ptr()], k_c.data_ptr(), stream=cur())

    def whiten_full():
        ctx.obs_whiten_device(nprof, nlev, m, se_p.data_ptr(), y.data_ptr(), fx.data_ptr(), [k_t.data_ptr(), k_h.data_ptr()],
                              lpk.data_ptr(), keep.data_ptr(), wstatus.data_ptr(), d_y_out=y_w.data_ptr(), d_fx_out=fx_w.data_ptr(),
                              d_k_out=[kw_t.data_ptr(), kw_h.data_ptr()], se_full=True, stream=cur())

    def whiten_r():
        ctx.obs_whiten_device(nprof, r, m, se_p.data_ptr(), y.data_ptr(), fx.data_ptr(), [k_c.data_ptr()], lpk.data_ptr(),
                              keep.data_ptr(), wstatus.data_ptr(), d_y_out=y_w.data_ptr(), d_fx_out=fx_w.data_ptr(),
                              d_k_out=[kw_c.data_ptr()], se_full=True, stream=cur())

    def torch_whiten(blocks, tag):
        rows = torch.isfinite(y) & torch.isfinite(fx)
        for b in blocks:
            rows = rows & torch.isfinite(b).all(dim=2)
        pair = rows[:, :, None] & rows[:, None, :]
        lt = torch.linalg.cholesky(torch.where(pair, se_p, torch.eye(m, **f64)[None]))
        vec = torch.stack([y, fx], dim=2).masked_fill(~rows[:, :, None], 0.0)
        held[tag] = [tri_solve(lt, b.masked_fill(~rows[:, :, None], 0.0), False) for b in blocks] + [
            tri_solve(lt, vec, False).masked_fill(~rows[:, :, None], float("nan")), lt]

    def apply_vec():
        ctx.obs_whiten_apply_device(nprof, 1, m, lpk.data_ptr(), keep.data_ptr(), mode=0, d_y=fx.data_ptr(), d_y_out=v_w.data_ptr(),
                                    stream=cur())

    def ungain(g, out):
        ctx.obs_whiten_apply_device(nprof, g.shape[2], m, lpk.data_ptr(), keep.data_ptr(), mode=1, d_k_in=[g.data_ptr()],
                                    d_k_out=[out.data_ptr()], stream=cur())

    def step_full(kt, kh, sev, yv, fv):
        ctx.oe_step_device(nprof, nlev, m, [kt.data_ptr(), kh.data_ptr()], x.data_ptr(), xa.data_ptr(), sa.data_ptr(),
                           sev.data_ptr(), yv.data_ptr(), fv.data_ptr(), x_new.data_ptr(), status.data_ptr(), xa_per_profile=True,
                           d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(), d_post_var=post_var.data_ptr(), d_nobs=nobs.data_ptr(),
                           stream=cur())

    def step_r(kc, sev, yv, fv):
        ctx.oe_step_device(nprof, r, m, [kc.data_ptr()], c.data_ptr(), c_a.data_ptr(), sa_c.data_ptr(), sev.data_ptr(),
                           yv.data_ptr(), fv.data_ptr(), c_new.data_ptr(), status.data_ptr(), d_chi2=chi2.data_ptr(),
                           d_dfs=dfs.data_ptr(), d_post_var=pv.data_ptr(), d_nobs=nobs.data_ptr(), stream=cur())

    k3t, k3h = k_t.reshape(nprof, m, nlev), k_h.reshape(nprof, m, nlev)
    project()
    whiten_full()
    torch_whiten([k3t, k3h], "full")
    torch.cuda.synchronize()
    lt_full = held["full"][-1]                                # torch's factor, for its own apply and un-whitening
    kept = keep.bool()

    paths = [("whiten_full", whiten_full), ("torch_whiten_full", lambda: torch_whiten([k3t, k3h], "full")),
             ("whiten_r32", whiten_r), ("torch_whiten_r32", lambda: torch_whiten([k_c], "r")),
             ("apply_vec", apply_vec),
             ("torch_apply_vec", lambda: held.__setitem__("v", tri_solve(
                 lt_full, fx.masked_fill(~kept, 0.0)[:, :, None], False))),
             ("ungain_full", lambda: ungain(gain_full, ug_full)),
             ("torch_ungain_full", lambda: held.__setitem__("gf", tri_solve(
                 lt_full.transpose(1, 2), gain_full.masked_fill(~kept[:, :, None], 0.0), True))),
             ("ungain_r32", lambda: ungain(gain_r, ug_r)),
             ("torch_ungain_r32", lambda: held.__setitem__("gr", tri_solve(
                 lt_full.transpose(1, 2), gain_r.masked_fill(~kept[:, :, None], 0.0), True))),
             ("iter_full", lambda: (k_matrix(), step_full(k_t, k_h, se, y, fx))),
             ("iter_full_se", lambda: (k_matrix(), whiten_full(), step_full(kw_t, kw_h, ones, y_w, fx_w))),
             ("iter_r32", lambda: (k_matrix(), project(), step_r(k_c, se, y, fx))),
             ("iter_r32_se", lambda: (k_matrix(), project(), whiten_r(), step_r(kw_c, ones, y_w, fx_w)))]
    inner = {name: max(1, a.inner) for name, _ in paths if not name.startswith("iter")}
    for _ in range(3):
        for _, fn in paths:
            fn()                                               # warm-up: code objects, LDS limits, torch's allocator
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in paths}
    for _ in range(a.reps):
        for name, fn in paths:                                 # alternately, in the same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            count = inner.get(name, 1)
            e0.record()
            for _ in range(count):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / count)
    res = {"shape": {"nprof": nprof, "nlev": nlev, "nblk": nblk, "m": m, "r": r, "model": "R24", "se": "full [nprof][m][m]",
                     "rows_dropped": int((~kept).sum().item())},
           "reps": a.reps, "torch_solve_triangular_profiles_per_call": chunk["profiles"], "calls_per_event_pair_short_paths": max(1, a.inner), "hbm_copy_tb_s": HBM_MEASURED_TB_S}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    for tag, cols in (("full", n), ("r32", r)):
        moved = 2 * 8.0 * nprof * m * cols                     # K in, K out
        sec = res[f"whiten_{tag}"]["median_ms"] * 1e-3
        fma = float(nprof) * (m * (m - 1) / 2) * (cols + 2)
        res[tag] = {"bytes_moved_k_in_and_out": moved, "gb_s": moved / sec / 1e9,
                    "share_of_copy_rate": moved / sec / (HBM_MEASURED_TB_S * 1e12), "time_at_copy_rate_ms": moved / (HBM_MEASURED_TB_S * 1e9),
                    "fma_of_the_substitutions": fma, "gfma_s": fma / sec / 1e9,
                    "ratio_whiten_over_torch": res[f"whiten_{tag}"]["median_ms"] / res[f"torch_whiten_{tag}"]["median_ms"],
                    "ratio_ungain_over_torch": res[f"ungain_{tag}"]["median_ms"] / res[f"torch_ungain_{tag}"]["median_ms"],
                    "iteration_with_se_over_without": res[f"iter_{tag}_se"]["median_ms"] / res[f"iter_{tag}"]["median_ms"]}
    res["ratio_apply_vec_over_torch"] = res["apply_vec"]["median_ms"] / res["torch_apply_vec"]["median_ms"]
    whiten_full()
    torch_whiten([k3t, k3h], "full")
    torch.cuda.synchronize()
    ok = (wstatus == 1)[:, None, None]
    ref = held["full"][0]
    res["largest_difference_whiten_vs_torch_of_column_max"] = float(
        (((kw_t.reshape(nprof, m, nlev) - ref).abs() / ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)) * ok).max())
    res["whiten_status_counts"] = {str(s): int((wstatus == s).sum().item()) for s in (1, 2, 3)}
    sb.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
