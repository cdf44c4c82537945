"""Device time of the characterisation entries (mwrt_oe_gain_device, mwrt_oe_product_device) next to the
merged step and to the same algebra in torch, one process, one stream, HIP events, at 1000 profiles x 180 levels x 2 blocks
(T, rh) x 98 observations (14 channels x 7 elevations), K from the device K-matrix call on the synthetic profiles:

  (a) gain_all      mwrt_oe_gain_device with every output
  (b) gain_only     mwrt_oe_gain_device with d_gain and d_keep alone
  (c) product_avk   mwrt_oe_product_device, A = gain K            (1000 x 360 x 360 out of 98 rows)
  (d) product_cov   mwrt_oe_product_device, S^ = Sa - gain W
  (e) oe_all        mwrt_oe_step_device with all diagnostics: the same passes over the panels less one triangular product
  (f) torch_gain    torch on the same buffers: cat, K Sa, bmm, linalg.cholesky, cholesky_solve -> gain^T
  (g) torch_avk     torch.bmm(gain, K) on the gain of (f)
  (h) torch_cov     Sa - torch.bmm(gain, W)

The eight are run alternately, repetition by repetition, each between one pair of HIP events on the current stream.
Usage: python tools/oe_char_time.py [--reps N] [--nprof N] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.Context(0)
    nprof, nlev, frq, ang = a.nprof, pr.N_LEVELS, pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
    nf, nang = frq.size, ang.size
    m, nblk = nf * nang, 2
    n = nblk * nlev
    f64 = dict(dtype=torch.float64, device="cuda")
    P = pr.synthetic_profiles(nprof, 2)
    z, p, t, rh = (torch.tensor(P[k], **f64) for k in ("z", "p", "t", "rh"))
    tb = torch.empty((nprof, nang, nf), **f64)
    k_t, k_h = (torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(2))
    valid = torch.empty(nprof, dtype=torch.uint8, device="cuda")
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
    sa, se = torch.tensor(sa_h, **f64), torch.full((m,), 0.25, **f64)
    x = torch.stack([t, rh], dim=1).contiguous()
    xa = (x + torch.tensor(rng.standard_normal((nprof, nblk, nlev)) * np.array([0.5, 0.02])[None, :, None], **f64)).contiguous()
    fx = tb.reshape(nprof, m)
    y = fx + torch.tensor(rng.standard_normal((nprof, m)) * 0.5, **f64)
    kp = [k_t.data_ptr(), k_h.data_ptr()]
    gain, ksa = torch.empty((nprof, m, n), **f64), torch.empty((nprof, m, n), **f64)
    keep = torch.empty((nprof, m), dtype=torch.uint8, device="cuda")
    avk_diag, noise_var, smooth_var = (torch.empty_like(x) for _ in range(3))
    dfs_block = torch.empty((nprof, nblk), **f64)
    nobs = torch.empty(nprof, dtype=torch.int32, device="cuda")
    status = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    out = torch.empty((nprof, n, n), **f64)
    x_new, post_var = torch.empty_like(x), torch.empty_like(x)
    chi2, dfs = torch.empty(nprof, **f64), torch.empty(nprof, **f64)

    def gain_entry(everything):
        extra = dict(d_ksa=ksa.data_ptr(), d_avk_diag=avk_diag.data_ptr(), d_dfs_block=dfs_block.data_ptr(),
                     d_noise_var=noise_var.data_ptr(), d_smooth_var=smooth_var.data_ptr(), d_nobs=nobs.data_ptr()) if everything else {}
        ctx.oe_gain_device(nprof, nlev, m, kp, x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(), y.data_ptr(),
                           fx.data_ptr(), status.data_ptr(), d_gain=gain.data_ptr(), d_keep=keep.data_ptr(),
                           xa_per_profile=True, stream=cur(), **extra)

    def product(which):
        ctx.oe_product_device(nprof, nlev, m, which, gain.data_ptr(), keep.data_ptr(), out.data_ptr(), kp,
                              d_ksa=ksa.data_ptr(), d_sa=sa.data_ptr(), stream=cur())

    def oe_all():
        ctx.oe_step_device(nprof, nlev, m, kp, x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(), y.data_ptr(),
                           fx.data_ptr(), x_new.data_ptr(), status.data_ptr(), d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(),
                           d_post_var=post_var.data_ptr(), d_nobs=nobs.data_ptr(), xa_per_profile=True, stream=cur())

    held = {}

    def torch_gain():
        K = torch.cat([k_t.reshape(nprof, m, nlev), k_h.reshape(nprof, m, nlev)], dim=2)       # [nprof][m][n]
        W = K @ sa
        G = torch.bmm(W, K.transpose(1, 2)) + torch.diag(se)
        held["K"], held["W"] = K, W
        held["g"] = torch.cholesky_solve(W, torch.linalg.cholesky(G))                          # gain^T [nprof][m][n]

    def torch_avk():
        held["avk"] = torch.bmm(held["g"].transpose(1, 2), held["K"])

    def torch_cov():
        held["cov"] = sa - torch.bmm(held["g"].transpose(1, 2), held["W"])

    paths = (("gain_all", lambda: gain_entry(True)), ("gain_only", lambda: gain_entry(False)),
             ("product_avk", lambda: product(nat.OE_PRODUCT_AVK)), ("product_cov", lambda: product(nat.OE_PRODUCT_POST_COV)),
             ("oe_all", oe_all), ("torch_gain", torch_gain), ("torch_avk", torch_avk), ("torch_cov", torch_cov))
    for _ in range(3):
        for _, fn in paths:
            fn()                                               # warm-up: code objects, small copies, torch's allocator
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in paths}
    for _ in range(a.reps):
        for name, fn in paths:                                 # alternately, in the same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"shape": {"nprof": nprof, "nlev": nlev, "nblk": nblk, "m": m, "model": "R24"}, "reps": a.reps,
           "mfma_variant": "not built: plain fp64 FMA only, no A/B exists"}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    gain_entry(True)
    product(nat.OE_PRODUCT_AVK)
    torch_gain()
    torch_avk()
    torch.cuda.synchronize()
    res["largest_difference_gain_vs_torch_of_max_abs"] = float((gain - held["g"]).abs().max() / held["g"].abs().max())
    res["largest_difference_avk_vs_torch_of_max_abs"] = float((out - held["avk"]).abs().max() / held["avk"].abs().max())
    res["status_counts"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
    res["mean_dfs_per_block"] = [float(v) for v in dfs_block.mean(dim=0)]
    med = lambda k: res[k]["median_ms"]   # noqa: E731
    res["product_gfma_per_s"] = {k: nprof * n * n * m / (med(k) * 1e-3) / 1e9 for k in ("product_avk", "product_cov")}
    res["product_write_gb_per_s"] = {k: nprof * n * n * 8 / (med(k) * 1e-3) / 1e9 for k in ("product_avk", "product_cov")}
    res["ratio_gain_all_over_oe_all"] = med("gain_all") / med("oe_all")
    res["ratio_gain_all_over_torch_gain"] = med("gain_all") / med("torch_gain")
    res["ratio_products_over_torch_products"] = (med("product_avk") + med("product_cov")) / (med("torch_avk") + med("torch_cov"))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
