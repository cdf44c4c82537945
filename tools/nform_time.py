"""Device time of the n-form of the optimal-estimation step (mwrt_oe_nform_*_device) beside the m-form path it
replaces for a reduced state, one process, one stream, HIP events, at the design shape: 1000 profiles x 180 levels x 2 blocks
(T, rh), K from the device K-matrix call on the synthetic profiles, 98 observations (14 channels x 7 elevations), r = 8, 32
and 64 leading eigenvectors of the prior covariance.  Per r, on the one block K B [nprof][98][r]:

  nf_prepare_rR       mwrt_oe_nform_prepare_device
  nf_solve_rR         mwrt_oe_nform_solve_device, x_new and status alone
  nf_solve_all_rR     ... with chi2, dfs, post_var and post_cov
  nf_cost_rR          mwrt_oe_nform_cost_device
  m_step_rR           mwrt_oe_step_device without diagnostics
  m_step_diag_rR      ... with chi2, dfs, nobs (post_var of the coefficients is not what the retrieval needs)
  m_gain_product_rR   mwrt_oe_gain_device + mwrt_oe_product_device (post_cov): what form="m" needs for a level-space post_var
  torch_rR            the n-form algebra in torch: bmm, cholesky, cholesky_solve, cholesky_inverse
  iter_n_rR           one reduced step WITH the level-space post_var (OneDVar.step(post_var=True) with a basis), form="n":
                      K-matrix call, projection, prepare, solve with post_cov, the contraction diag(B S^ B^T)
  iter_m_rR           ... form="m": K-matrix call, projection, step with diagnostics, gain, product, the contraction
  retrieve_n_rR       one iteration of OneDVar.retrieve with a basis, whose steps skip post_var, form="n": K-matrix call,
                      projection, prepare, solve with chi2 and dfs
  retrieve_m_rR       ... form="m": K-matrix call, projection, step with diagnostics (what tools/basis_time.py calls reduced_rR,
                      less its post_var of the coefficients)
and, at r = 32 on a synthetic K of the same statistics, prepare alone at m = 140 and m = 896 (14 x 64 elevations) with the
bytes it must move (K once, y, fx, keep, H, g) against the device's copy rate measured in the same session: ``copy`` is
torch's device-to-device copy of a 1 GiB float64 buffer, interleaved with the other paths, 2 GiB moved per call.  The torch
algebra is published only where its x agrees with the device's to 1e-6 of the largest move; ``torch_check_rR`` holds the
differences of its K^T W K and K^T W r from the device's H and g and the residuals of its factor, of cholesky_solve and of
linalg.solve on its own matrices, so a disagreement names its step.

All paths are run alternately, repetition by repetition, each between one pair of HIP events on the current stream; a short
path brackets ``--inner`` back-to-back calls and the time is divided by that.  Median [p10 - p90] of ``--reps`` repetitions
after warm-up.  Usage: python tools/nform_time.py [--reps N] [--inner N] [--nprof N] [--out FILE.json]"""
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

COPY_BYTES = 1 << 30
TORCH_AGREES = 1e-6
RANKS = (8, 32, 64)
LONG_M = (140, 896)


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
    m, nblk = nf * nang, 2
    n = nblk * nlev
    f64 = dict(dtype=torch.float64, device="cuda")
    u8 = dict(dtype=torch.uint8, device="cuda")
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
    rng = np.random.default_rng(2000)
    lev = np.arange(nlev)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / (nlev / 6.0))
    sa_h = np.zeros((n, n))
    sa_h[:nlev, :nlev] = 2.0 ** 2 * corr
    sa_h[nlev:, nlev:] = 0.1 ** 2 * corr
    sa_h[:nlev, nlev:] = 0.3 * 2.0 * 0.1 * corr
    sa_h[nlev:, :nlev] = sa_h[:nlev, nlev:].T
    se = torch.full((m,), 0.25, **f64)
    fx = tb.reshape(nprof, m)
    y = fx + torch.tensor(rng.standard_normal((nprof, m)) * 0.5, **f64)
    chi2, dfs, cost = (torch.empty(nprof, **f64) for _ in range(3))
    nobs = torch.empty(nprof, dtype=torch.int32, device="cuda")
    status = torch.empty(nprof, **u8)

    def lin_buffers(r, rows):
        return dict(h=torch.empty((nprof, r * (r + 1) // 2), **f64), g=torch.empty((nprof, r), **f64), rwr=torch.empty(nprof, **f64),
                    keep=torch.empty((nprof, rows), **u8), nobs=torch.empty(nprof, dtype=torch.int32, device="cuda"),
                    lin_status=torch.empty(nprof, **u8))

    per_rank, paths, inner, held = {}, [], {}, {}
    for r in RANKS:
        sb = StateBasis.from_covariance(torch.tensor(sa_h), r)
        _, handle = sb.native_handle(nblk, 0)
        b = sb.b.to("cuda")
        sa_c = sb.sa_c.to("cuda").contiguous()
        q = dict(sb=sb, handle=handle, b=b, sa_c=sa_c, sa_inv=torch.linalg.inv(sa_c).contiguous(),
                 k_c=torch.empty((nprof, m, r), **f64), c=torch.zeros((nprof, 1, r), **f64), c_a=torch.zeros((1, r), **f64),
                 c_new=torch.empty((nprof, 1, r), **f64), pv=torch.empty((nprof, 1, r), **f64), pc=torch.empty((nprof, r, r), **f64),
                 gain=torch.empty((nprof, m, r), **f64), ksa=torch.empty((nprof, m, r), **f64), keep=torch.empty((nprof, m), **u8),
                 lin=lin_buffers(r, m))
        per_rank[r] = q

        def project(q=q):
            ctx.basis_project_device(q["handle"], nprof, m, [k_t.data_ptr(), k_h.data_ptr()], q["k_c"].data_ptr(), stream=cur())

        def nf_prepare(q=q, r=r):
            lin = q["lin"]
            ctx.oe_nform_prepare_device(nprof, r, m, [q["k_c"].data_ptr()], q["c"].data_ptr(), q["c_a"].data_ptr(), se.data_ptr(),
                                        y.data_ptr(), fx.data_ptr(), lin["h"].data_ptr(), lin["g"].data_ptr(), lin["rwr"].data_ptr(),
                                        lin["keep"].data_ptr(), lin["nobs"].data_ptr(), lin["lin_status"].data_ptr(), stream=cur())

        def nf_solve(q=q, r=r, every=False, post_cov=False, chi2_dfs=False):
            lin = q["lin"]
            opt = dict(d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr()) if every or post_cov or chi2_dfs else {}
            if every:
                opt["d_post_var"] = q["pv"].data_ptr()
            if every or post_cov:
                opt["d_post_cov"] = q["pc"].data_ptr()
            ctx.oe_nform_solve_device(nprof, r, m, 1, q["c"].data_ptr(), q["c_a"].data_ptr(), q["sa_inv"].data_ptr(), lin["h"].data_ptr(),
                                      lin["g"].data_ptr(), lin["rwr"].data_ptr(), lin["lin_status"].data_ptr(), q["c_new"].data_ptr(),
                                      status.data_ptr(), stream=cur(), **opt)

        def nf_cost(q=q, r=r):
            ctx.oe_nform_cost_device(nprof, r, m, 1, q["c"].data_ptr(), q["c_a"].data_ptr(), q["sa_inv"].data_ptr(), se.data_ptr(),
                                     y.data_ptr(), fx.data_ptr(), q["lin"]["keep"].data_ptr(), cost.data_ptr(), stream=cur())

        def m_step(q=q, r=r, diag=False):
            opt = dict(d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(), d_nobs=nobs.data_ptr()) if diag else {}
            ctx.oe_step_device(nprof, r, m, [q["k_c"].data_ptr()], q["c"].data_ptr(), q["c_a"].data_ptr(), q["sa_c"].data_ptr(),
                               se.data_ptr(), y.data_ptr(), fx.data_ptr(), q["c_new"].data_ptr(), status.data_ptr(), stream=cur(), **opt)

        def m_gain_product(q=q, r=r):
            ctx.oe_gain_device(nprof, r, m, [q["k_c"].data_ptr()], q["c"].data_ptr(), q["c_a"].data_ptr(), q["sa_c"].data_ptr(),
                               se.data_ptr(), y.data_ptr(), fx.data_ptr(), status.data_ptr(), d_gain=q["gain"].data_ptr(),
                               d_ksa=q["ksa"].data_ptr(), d_keep=q["keep"].data_ptr(), stream=cur())
            ctx.oe_product_device(nprof, r, m, nat.OE_PRODUCT_POST_COV, q["gain"].data_ptr(), q["keep"].data_ptr(), q["pc"].data_ptr(),
                                  [None], d_ksa=q["ksa"].data_ptr(), d_sa=q["sa_c"].data_ptr(), stream=cur())

        def contraction(q=q, r=r):
            held[r] = torch.einsum("kj,pji,ki->pk", q["b"], q["pc"], q["b"])

        def torch_nform(q=q, r=r):
            k = q["k_c"]
            kw = k / se[None, :, None]
            c_mat = torch.bmm(kw.transpose(1, 2), k) + q["sa_inv"][None]
            rhs = torch.bmm(kw.transpose(1, 2), (y - fx)[:, :, None]) - (q["sa_inv"] @ (q["c"][:, 0] - q["c_a"]).T).T[:, :, None]
            chol = torch.linalg.cholesky(c_mat)
            held[("x", r)] = q["c"][:, 0] + torch.cholesky_solve(rhs, chol)[:, :, 0]
            held[("s", r)] = torch.cholesky_inverse(chol)
            held[("parts", r)] = (c_mat, rhs, chol)

        def iter_n(q=q, r=r, project=project, nf_prepare=nf_prepare, nf_solve=nf_solve, contraction=contraction):
            k_matrix()
            project()
            nf_prepare()
            nf_solve(post_cov=True)
            contraction()

        def iter_m(q=q, r=r, project=project, m_step=m_step, m_gain_product=m_gain_product, contraction=contraction):
            k_matrix()
            project()
            m_step(diag=True)
            m_gain_product()
            contraction()

        def retrieve_n(project=project, nf_prepare=nf_prepare, nf_solve=nf_solve):
            k_matrix()
            project()
            nf_prepare()
            nf_solve(chi2_dfs=True)

        def retrieve_m(project=project, m_step=m_step):
            k_matrix()
            project()
            m_step(diag=True)

        project()
        short = [(f"nf_prepare_r{r}", nf_prepare), (f"nf_solve_r{r}", nf_solve),
                 (f"nf_solve_all_r{r}", lambda nf_solve=nf_solve: nf_solve(every=True)), (f"nf_cost_r{r}", nf_cost),
                 (f"m_step_r{r}", m_step), (f"m_step_diag_r{r}", lambda m_step=m_step: m_step(diag=True)),
                 (f"m_gain_product_r{r}", m_gain_product), (f"torch_r{r}", torch_nform)]
        for name, _ in short:
            inner[name] = max(1, a.inner)
        paths += short + [(f"iter_n_r{r}", iter_n), (f"iter_m_r{r}", iter_m), (f"retrieve_n_r{r}", retrieve_n),
                          (f"retrieve_m_r{r}", retrieve_m)]

    # prepare alone on many observations: a synthetic K B of the statistics of the real one at r = 32
    r_long = 32
    q32 = per_rank[r_long]
    long_bufs = {}
    for ml in LONG_M:
        scale = q32["k_c"].std(dim=(0, 1))
        kl = (torch.randn((nprof, ml, r_long), **f64) * scale[None, None, :]).contiguous()
        fl = 250.0 + 20.0 * torch.randn((nprof, ml), **f64)
        yl = fl + 0.5 * torch.randn((nprof, ml), **f64)
        sel = torch.full((ml,), 0.25, **f64)
        lin = lin_buffers(r_long, ml)
        long_bufs[ml] = (kl, yl, fl, sel, lin)

        def prepare_long(ml=ml, kl=kl, yl=yl, fl=fl, sel=sel, lin=lin):
            ctx.oe_nform_prepare_device(nprof, r_long, ml, [kl.data_ptr()], q32["c"].data_ptr(), q32["c_a"].data_ptr(), sel.data_ptr(),
                                        yl.data_ptr(), fl.data_ptr(), lin["h"].data_ptr(), lin["g"].data_ptr(), lin["rwr"].data_ptr(),
                                        lin["keep"].data_ptr(), lin["nobs"].data_ptr(), lin["lin_status"].data_ptr(), stream=cur())

        paths.append((f"nf_prepare_r{r_long}_m{ml}", prepare_long))
        inner[f"nf_prepare_r{r_long}_m{ml}"] = max(1, a.inner)

    # the copy rate of this device, this session: one read and one write of COPY_BYTES
    src = torch.empty(COPY_BYTES // 8, **f64).normal_()
    dst = torch.empty_like(src)
    paths.append(("copy", lambda: dst.copy_(src)))

    for _ in range(3):
        for _, fn in paths:
            fn()                                               # warm-up: code objects, LDS limits, torch's allocator and solvers
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
    res = {"shape": {"nprof": nprof, "nlev": nlev, "nblk": nblk, "m": m, "ranks": list(RANKS), "model": "R24"}, "reps": a.reps,
           "calls_per_event_pair_short_paths": max(1, a.inner)}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
    copy_tb_s = 2.0 * COPY_BYTES / (res["copy"]["median_ms"] * 1e-3) / 1e12
    res["copy"].update(bytes_moved=2.0 * COPY_BYTES, tb_s=copy_tb_s)
    for r in RANKS:
        q = per_rank[r]
        # the two forms' x_new on the same inputs, and the torch algebra, for the record
        per_rank[r]["lin"]["h"].zero_()
        [fn for nm, fn in paths if nm == f"nf_prepare_r{r}"][0]()
        [fn for nm, fn in paths if nm == f"nf_solve_r{r}"][0]()
        x_n = q["c_new"].clone()
        [fn for nm, fn in paths if nm == f"m_step_r{r}"][0]()
        [fn for nm, fn in paths if nm == f"torch_r{r}"][0]()
        torch.cuda.synchronize()
        unit = float((q["c_new"] - q["c_a"]).abs().max())
        c_mat, rhs, chol = held[("parts", r)]
        norm = lambda v: float(v.abs().amax())               # noqa: E731
        x_cs, x_ls = torch.cholesky_solve(rhs, chol), torch.linalg.solve(c_mat, rhs)
        il = torch.tril_indices(r, r, device="cuda")
        h_torch = (c_mat - q["sa_inv"][None])[:, il[0], il[1]]   # the packed lower triangle, row by row, as the device writes H
        res[f"torch_check_r{r}"] = {
            "h_minus_device_h_over_largest": norm(h_torch - q["lin"]["h"]) / norm(q["lin"]["h"]),
            "rhs_minus_device_g_over_largest": norm(rhs[:, :, 0] - q["lin"]["g"]) / norm(q["lin"]["g"]),
            "factor_residual": norm(torch.bmm(chol, chol.transpose(1, 2)) - c_mat) / norm(c_mat),
            "cholesky_solve_residual": norm(torch.bmm(c_mat, x_cs) - rhs) / norm(rhs),
            "linalg_solve_residual": norm(torch.bmm(c_mat, x_ls) - rhs) / norm(rhs),
            "cholesky_solve_minus_linalg_solve_over_largest": norm(x_cs - x_ls) / norm(x_ls),
            "finite": bool(torch.isfinite(chol).all() and torch.isfinite(x_cs).all()),
            # the x of the timed sequence (cholesky_solve queued straight behind cholesky) against the same call made
            # here, after a device synchronise, on the same factor and right-hand side
            "x_in_sequence_minus_x_after_synchronise_over_largest": norm(held[("x", r)] - q["c"][:, 0] - x_cs[:, :, 0]) / norm(x_cs)}
        torch_err = float((x_n[:, 0] - held[("x", r)]).abs().max()) / unit
        # the profile where torch and the device differ most, solved once more on the host from the device's H and g
        worst = int((x_n[:, 0] - held[("x", r)]).abs().amax(dim=1).argmax())
        h_full = np.zeros((r, r))
        h_full[np.tril_indices(r)] = q["lin"]["h"][worst].cpu().numpy()
        h_full = h_full + np.tril(h_full, -1).T
        x_host = np.linalg.solve(h_full + q["sa_inv"].cpu().numpy(), q["lin"]["g"][worst].cpu().numpy())
        res[f"torch_check_r{r}"].update(
            worst_profile=worst, device_status=int(status[worst]),
            host_minus_device_over_largest_move=float(np.abs(x_host - x_n[worst, 0].cpu().numpy()).max()) / unit,
            host_minus_torch_over_largest_move=float(np.abs(x_host - held[("x", r)][worst].cpu().numpy()).max()) / unit,
            largest_move_of_worst_profile_over_batch_largest=float(np.abs(x_host).max()) / unit)
        if not torch_err <= TORCH_AGREES:                    # a baseline that computes something else is no baseline
            res[f"torch_r{r}"] = {"median_ms": None, "withheld": "its x differs from the device's by %.3g of the largest move" % torch_err}
        res[f"r{r}"] = {
            "ratio_iter_n_over_iter_m": res[f"iter_n_r{r}"]["median_ms"] / res[f"iter_m_r{r}"]["median_ms"],
            "ratio_retrieve_n_over_retrieve_m": res[f"retrieve_n_r{r}"]["median_ms"] / res[f"retrieve_m_r{r}"]["median_ms"],
            "update_n_ms": res[f"nf_prepare_r{r}"]["median_ms"] + res[f"nf_solve_all_r{r}"]["median_ms"],
            "update_m_ms": res[f"m_step_diag_r{r}"]["median_ms"] + res[f"m_gain_product_r{r}"]["median_ms"],
            "x_new_n_minus_m_over_largest_move": float((x_n - q["c_new"]).abs().max()) / unit,
            "x_new_n_minus_torch_over_largest_move": torch_err}
        q["sb"].close()
    for ml in LONG_M:
        moved = 8.0 * nprof * (ml * r_long + 2 * ml + r_long * (r_long + 1) // 2 + r_long + 1) + nprof * ml + 8.0 * ml
        sec = res[f"nf_prepare_r{r_long}_m{ml}"]["median_ms"] * 1e-3
        res[f"prepare_m{ml}"] = {"bytes_moved": moved, "gb_s": moved / sec / 1e9,
                                 "share_of_copy_rate": moved / sec / (copy_tb_s * 1e12),
                                 "fma": float(nprof) * ml * r_long * (r_long + 1) / 2, "gfma_s": float(nprof) * ml * r_long * (r_long + 1) / 2 / sec / 1e9}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
