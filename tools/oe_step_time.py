"""Device time of the optimal-estimation step (mwrt_oe_step_device) next to what a caller did before, one
process, one stream, HIP events, at 1000 profiles x 180 levels x 2 blocks (T, rh) x 98 observations (14 channels x 7
elevations), K from the device K-matrix call on the synthetic profiles:

  (a) oe_x_only   mwrt_oe_step_device, x_new and status only
  (b) oe_all      (a) plus chi2, dfs, post_var, nobs
  (c) torch       the same step on the same device buffers with torch: cat, bmm, linalg.cholesky, cholesky_solve
  (d) k_matrix    the mwrt_tb_jacobian_batch_vars_device call that produces K, for scale

The four are run alternately, repetition by repetition, each between one pair of HIP events on the current stream.
Usage: python tools/oe_step_time.py [--reps N] [--nprof N] [--out FILE.json]"""
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
    sa, se = torch.tensor(sa_h, **f64), torch.full((m,), 0.25, **f64)
    x = torch.stack([t, rh], dim=1).contiguous()
    xa = (x + torch.tensor(rng.standard_normal((nprof, nblk, nlev)) * np.array([0.5, 0.02])[None, :, None], **f64)).contiguous()
    fx = tb.reshape(nprof, m)
    y = fx + torch.tensor(rng.standard_normal((nprof, m)) * 0.5, **f64)
    x_new, post_var = torch.empty_like(x), torch.empty_like(x)
    chi2, dfs = torch.empty(nprof, **f64), torch.empty(nprof, **f64)
    nobs = torch.empty(nprof, dtype=torch.int32, device="cuda")
    status = torch.empty(nprof, dtype=torch.uint8, device="cuda")

    def oe(diagnostics):
        extra = dict(d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(), d_post_var=post_var.data_ptr(),
                     d_nobs=nobs.data_ptr()) if diagnostics else {}
        ctx.oe_step_device(nprof, nlev, m, [k_t.data_ptr(), k_h.data_ptr()], x.data_ptr(), xa.data_ptr(), sa.data_ptr(),
                           se.data_ptr(), y.data_ptr(), fx.data_ptr(), x_new.data_ptr(), status.data_ptr(),
                           xa_per_profile=True, stream=cur(), **extra)

    def torch_step():
        K = torch.cat([k_t.reshape(nprof, m, nlev), k_h.reshape(nprof, m, nlev)], dim=2)       # [nprof][m][n]
        W = K @ sa
        G = torch.bmm(W, K.transpose(1, 2)) + torch.diag(se)
        d = (y - fx) + torch.bmm(K, (x - xa).reshape(nprof, n, 1)).squeeze(2)
        L = torch.linalg.cholesky(G)
        u = torch.cholesky_solve(d.unsqueeze(2), L)
        return xa + torch.bmm(W.transpose(1, 2), u).reshape(nprof, nblk, nlev)

    paths = (("oe_x_only", lambda: oe(False)), ("oe_all", lambda: oe(True)), ("torch", torch_step), ("k_matrix", k_matrix))
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
    oe(True)
    ref = torch_step()
    torch.cuda.synchronize()
    scale = (ref - xa).abs().amax(dim=2, keepdim=True)
    res["largest_difference_oe_vs_torch_of_block_scale"] = float(((x_new - ref).abs() / scale).max())
    res["status_counts"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
    res["mean_dfs"], res["mean_chi2_over_m"] = float(dfs.mean()), float((chi2 / m).mean())
    res["ratio_oe_x_only_over_torch"] = res["oe_x_only"]["median_ms"] / res["torch"]["median_ms"]
    res["ratio_oe_x_only_over_k_matrix"] = res["oe_x_only"]["median_ms"] / res["k_matrix"]["median_ms"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
