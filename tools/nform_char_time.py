"""Device time of the characterisation of the n-form step (mwrt_oe_nform_char_device, mwrt_oe_nform_gain_device, DESIGN
4.11.1) beside the m-form route it stands in for and beside the same algebra in torch: one process, one stream, HIP events, at
the design shape: 1000 profiles x 180 levels x 2 blocks (T, rh), K from the device K-matrix call on the synthetic profiles,
98 observations (14 channels x 7 elevations), projected on the r = 8, 32 and 64 leading eigenvectors of the prior covariance.
Per r, on the one block K B [nprof][98][r] and its n-form linearisation:

  nfc_char_diag_rR      mwrt_oe_nform_char_device, avk_diag and dfs_block alone
  nfc_char_budget_rR    ... with noise_var and smooth_var (every row of A is formed, none leaves the workgroup)
  nfc_char_all_rR       ... with d_post_cov and the full d_avk as well
  nfc_gain_rR           mwrt_oe_nform_gain_device
  m_char_rR             the m-form route: mwrt_oe_gain_device (every output) + mwrt_oe_product_device twice (avk, post_cov)
  torch_char_rR         the algebra in torch: K^T W K, cholesky, cholesky_inverse, S^ H, the two diagonals, W K S^
and, on a synthetic K B of the same statistics at m = 224 and m = 896 (the m-form refuses both), prepare, nfc_gain and the
torch gain (W K S^ alone).  For the gain kernel ``gain_*`` holds the bytes it must move (K once, the gain once, S^ once per
profile, keep and se) against the device's copy rate measured in the same session: ``copy`` is torch's device-to-device
copy of a 1 GiB float64 buffer, interleaved with the other paths, 2 GiB moved per call.  ``check_rR`` holds the largest
difference of the torch algebra and of the m-form route from the n-form entries, so a baseline that computes something else
shows.

All paths are run alternately, repetition by repetition, each between one pair of HIP events on the current stream; a short
path brackets ``--inner`` back-to-back calls and the time is divided by that.  Median [p10 - p90] of ``--reps`` repetitions
after warm-up.  Usage: python tools/nform_char_time.py [--reps N] [--inner N] [--nprof N] [--out FILE.json]"""
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
RANKS = (8, 32, 64)
LONG_M = (224, 896)


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
    cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    ctx.tb_jacobian_batch_vars_device("R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang,
                                      tb.data_ptr(), k_t.data_ptr(), k_h.data_ptr(), valid.data_ptr(),
                                      variables=nat.JacVariables.of(humidity="rh"), stream=cur())
    torch.cuda.synchronize()
    rng = np.random.default_rng(2000)
    lev = np.arange(nlev)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / (nlev / 6.0))
    sa_h = np.zeros((n, n))
    sa_h[:nlev, :nlev] = 2.0 ** 2 * corr
    sa_h[nlev:, nlev:] = 0.1 ** 2 * corr
    sa_h[:nlev, nlev:] = 0.3 * 2.0 * 0.1 * corr
    sa_h[nlev:, :nlev] = sa_h[:nlev, nlev:].T
    fx = tb.reshape(nprof, m)
    y = fx + torch.tensor(rng.standard_normal((nprof, m)) * 0.5, **f64)

    def buffers(r, rows):
        return dict(h=torch.empty((nprof, r * (r + 1) // 2), **f64), g=torch.empty((nprof, r), **f64), rwr=torch.empty(nprof, **f64),
                    keep=torch.empty((nprof, rows), **u8), nobs=torch.empty(nprof, dtype=torch.int32, device="cuda"),
                    lin_status=torch.empty(nprof, **u8), status=torch.empty(nprof, **u8), post_cov=torch.empty((nprof, r, r), **f64),
                    avk=torch.empty((nprof, r, r), **f64), avk_diag=torch.empty((nprof, r), **f64), noise=torch.empty((nprof, r), **f64),
                    smooth=torch.empty((nprof, r), **f64), dfs_block=torch.empty((nprof, 1), **f64),
                    gain=torch.empty((nprof, rows, r), **f64), se=torch.full((rows,), 0.25, **f64))

    paths, inner, held, cases = [], {}, {}, {}
    for r in RANKS:
        sb = StateBasis.from_covariance(torch.tensor(sa_h), r)
        _, handle = sb.native_handle(nblk, 0)
        sa_c = sb.sa_c.to("cuda").contiguous()
        sa_inv = torch.linalg.inv(sa_c).contiguous()
        c, c_a = torch.zeros((nprof, 1, r), **f64), torch.zeros((1, r), **f64)
        k_c = torch.empty((nprof, m, r), **f64)
        ctx.basis_project_device(handle, nprof, m, [k_t.data_ptr(), k_h.data_ptr()], k_c.data_ptr(), stream=cur())
        torch.cuda.synchronize()
        sb.close()
        scale = k_c.std(dim=(0, 1))
        for rows in (m,) + LONG_M:
            if rows == m:
                kk, yy, ff = k_c, y, fx
            else:                                              # a synthetic K B of the statistics of the real one
                kk = (torch.randn((nprof, rows, r), **f64) * scale[None, None, :]).contiguous()
                ff = 250.0 + 20.0 * torch.randn((nprof, rows), **f64)
                yy = ff + 0.5 * torch.randn((nprof, rows), **f64)
            q = dict(buffers(r, rows), k=kk, y=yy, fx=ff, sa_inv=sa_inv, sa_c=sa_c, c=c, c_a=c_a, r=r, m=rows,
                     ksa=torch.empty((nprof, rows, r), **f64) if rows == m else None)
            cases[(r, rows)] = q

            def prepare(q=q):
                ctx.oe_nform_prepare_device(nprof, q["r"], q["m"], [q["k"].data_ptr()], q["c"].data_ptr(), q["c_a"].data_ptr(),
                                            q["se"].data_ptr(), q["y"].data_ptr(), q["fx"].data_ptr(), q["h"].data_ptr(), q["g"].data_ptr(),
                                            q["rwr"].data_ptr(), q["keep"].data_ptr(), q["nobs"].data_ptr(), q["lin_status"].data_ptr(),
                                            stream=cur())

            def char(q=q, budget=False, every=False):
                opt = dict(d_noise_var=q["noise"].data_ptr(), d_smooth_var=q["smooth"].data_ptr()) if budget or every else {}
                if every:
                    opt.update(d_post_cov=q["post_cov"].data_ptr(), d_avk=q["avk"].data_ptr())
                ctx.oe_nform_char_device(nprof, q["r"], q["m"], 1, q["sa_inv"].data_ptr(), q["h"].data_ptr(), q["lin_status"].data_ptr(),
                                         q["status"].data_ptr(), d_avk_diag=q["avk_diag"].data_ptr(), d_dfs_block=q["dfs_block"].data_ptr(),
                                         stream=cur(), **opt)

            def gain(q=q):
                ctx.oe_nform_gain_device(nprof, q["r"], q["m"], [q["k"].data_ptr()], q["se"].data_ptr(), q["keep"].data_ptr(),
                                         q["post_cov"].data_ptr(), q["status"].data_ptr(), q["gain"].data_ptr(), stream=cur())

            def torch_gain(q=q):
                held[("gain", q["r"], q["m"])] = torch.bmm(q["k"] / q["se"][None, :, None], q["post_cov"])

            prepare()
            char(every=True)                                   # S^ and the status the gain reads
            tag = f"r{r}" if rows == m else f"r{r}_m{rows}"
            short = [(f"nfc_gain_{tag}", gain)]
            if rows == m:
                def m_char(q=q):
                    ctx.oe_gain_device(nprof, q["r"], q["m"], [q["k"].data_ptr()], q["c"].data_ptr(), q["c_a"].data_ptr(), q["sa_c"].data_ptr(),
                                       q["se"].data_ptr(), q["y"].data_ptr(), q["fx"].data_ptr(), q["status_m"].data_ptr(),
                                       d_gain=q["gain_m"].data_ptr(), d_ksa=q["ksa"].data_ptr(), d_keep=q["keep_m"].data_ptr(),
                                       d_avk_diag=q["avk_diag_m"].data_ptr(), d_dfs_block=q["dfs_block_m"].data_ptr(),
                                       d_noise_var=q["noise_m"].data_ptr(), d_smooth_var=q["smooth_m"].data_ptr(), stream=cur())
                    for product, out in ((nat.OE_PRODUCT_AVK, q["avk_m"]), (nat.OE_PRODUCT_POST_COV, q["post_cov_m"])):
                        ctx.oe_product_device(nprof, q["r"], q["m"], product, q["gain_m"].data_ptr(), q["keep_m"].data_ptr(), out.data_ptr(),
                                              [q["k"].data_ptr()], d_ksa=q["ksa"].data_ptr(), d_sa=q["sa_c"].data_ptr(), stream=cur())

                def torch_char(q=q):
                    k = q["k"]
                    kw = k / q["se"][None, :, None]
                    h = torch.bmm(kw.transpose(1, 2), k)
                    s = torch.cholesky_inverse(torch.linalg.cholesky(h + q["sa_inv"][None]))
                    avk = torch.bmm(s, h)
                    noise = torch.einsum("pjk,pkj->pj", avk, s)
                    held[("char", q["r"])] = dict(post_cov=s, avk=avk, avk_diag=torch.diagonal(avk, dim1=1, dim2=2), noise=noise,
                                                  smooth=torch.diagonal(s, dim1=1, dim2=2) - noise, gain=torch.bmm(kw, s))

                for key in ("status", "keep", "gain", "avk_diag", "dfs_block", "noise", "smooth", "avk", "post_cov"):
                    q[key + "_m"] = torch.empty_like(q[key])
                short += [(f"nfc_char_diag_{tag}", char), (f"nfc_char_budget_{tag}", lambda char=char: char(budget=True)),
                          (f"nfc_char_all_{tag}", lambda char=char: char(every=True)), (f"m_char_{tag}", m_char),
                          (f"torch_char_{tag}", torch_char)]
            else:
                short += [(f"nf_prepare_{tag}", prepare), (f"torch_gain_{tag}", torch_gain)]
            for name, _ in short:
                inner[name] = max(1, a.inner)
            paths += short

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
    res = {"shape": {"nprof": nprof, "nlev": nlev, "nblk": nblk, "m": m, "ranks": list(RANKS), "long_m": list(LONG_M), "model": "R24"},
           "reps": a.reps, "calls_per_event_pair_short_paths": max(1, a.inner)}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
    copy_tb_s = 2.0 * COPY_BYTES / (res["copy"]["median_ms"] * 1e-3) / 1e12
    res["copy"].update(bytes_moved=2.0 * COPY_BYTES, tb_s=copy_tb_s)
    norm = lambda v: float(v.abs().amax())                     # noqa: E731
    for r in RANKS:
        q = cases[(r, m)]
        for name, fn in paths:                                 # once more, everything asked for, for the comparison
            if name in (f"nfc_char_all_r{r}", f"nfc_gain_r{r}", f"m_char_r{r}", f"torch_char_r{r}"):
                fn()
        torch.cuda.synchronize()
        th = held[("char", r)]
        res[f"check_r{r}"] = {
            "status_all_1": bool((q["status"] == 1).all() and (q["status_m"] == 1).all()),
            **{f"torch_{key}_over_largest": norm(th[key] - q[key]) / norm(q[key]) for key in ("post_cov", "avk", "avk_diag", "noise", "smooth", "gain")},
            **{f"m_form_{key}_over_largest": norm(q[key + "_m"] - q[key]) / norm(q[key])
               for key in ("post_cov", "avk", "avk_diag", "noise", "smooth", "gain", "dfs_block")}}
        res[f"r{r}"] = {
            "n_form_ms": res[f"nfc_char_all_r{r}"]["median_ms"] + res[f"nfc_gain_r{r}"]["median_ms"],
            "m_form_ms": res[f"m_char_r{r}"]["median_ms"], "torch_ms": res[f"torch_char_r{r}"]["median_ms"]}
        res[f"r{r}"]["ratio_n_over_m"] = res[f"r{r}"]["n_form_ms"] / res[f"r{r}"]["m_form_ms"]
        res[f"r{r}"]["ratio_n_over_torch"] = res[f"r{r}"]["n_form_ms"] / res[f"r{r}"]["torch_ms"]
        for rows in (m,) + LONG_M:
            tag = f"r{r}" if rows == m else f"r{r}_m{rows}"
            moved = 8.0 * nprof * (2 * rows * r + r * r) + nprof * rows + 8.0 * rows + nprof
            sec = res[f"nfc_gain_{tag}"]["median_ms"] * 1e-3
            res[f"gain_{tag}"] = {"bytes_moved": moved, "gb_s": moved / sec / 1e9, "share_of_copy_rate": moved / sec / (copy_tb_s * 1e12),
                                  "fma": float(nprof) * rows * r * r, "gfma_s": float(nprof) * rows * r * r / sec / 1e9}
            if rows != m:
                res[f"gain_{tag}"]["ratio_over_torch"] = res[f"nfc_gain_{tag}"]["median_ms"] / res[f"torch_gain_{tag}"]["median_ms"]
                ql = cases[(r, rows)]
                res[f"gain_{tag}"]["torch_minus_device_over_largest"] = norm(held[("gain", r, rows)] - ql["gain"]) / norm(ql["gain"])
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
