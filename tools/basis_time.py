"""Device time of the reduced-basis projection (mwrt_basis_project_device) and of the retrieval iteration it
makes possible, one process, one stream, HIP events, at the design shape: 1000 profiles x 180 levels x 2 blocks (T, rh) x 98
observations (14 channels x 7 elevations), K from the device K-matrix call on the synthetic profiles, r = 8, 32 and 64
leading eigenvectors of the prior covariance.  Per r:

  (a) project_rR    mwrt_basis_project_device: both K blocks -> K B [nprof][98][r]
  (b) torch_rR      the same product in torch on the same buffers: two matmul calls and an add
  (c) reduced_rR    one reduced iteration: the K-matrix call, (a), and mwrt_oe_step_device on the one block with every
                    diagnostic (nblk = 1, nlev = r)
and once
  (d) full          one full-state iteration on the same buffers: the K-matrix call and mwrt_oe_step_device with every
                    diagnostic at n = 360

All paths are run alternately, repetition by repetition, each between one pair of HIP events on the current stream; (a) and
(b) are short, so a pair of events brackets ``--inner`` back-to-back calls and the time is divided by that.  The file also
holds the bytes (a) must move, computed from the shapes, the resulting GB/s and its share of the 6.29 TB/s a float4 copy
reaches on an MI355X (the figure tools/obs_apply_time.py uses), and its FMA rate.
Usage: python tools/basis_time.py [--reps N] [--inner N] [--nprof N] [--out FILE.json]"""
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
RANKS = (8, 32, 64)


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
    chi2, dfs = torch.empty(nprof, **f64), torch.empty(nprof, **f64)
    nobs = torch.empty(nprof, dtype=torch.int32, device="cuda")
    status = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    x_new, post_var = torch.empty_like(x), torch.empty_like(x)

    def full():
        k_matrix()
        ctx.oe_step_device(nprof, nlev, m, [k_t.data_ptr(), k_h.data_ptr()], x.data_ptr(), xa.data_ptr(), sa.data_ptr(),
                           se.data_ptr(), y.data_ptr(), fx.data_ptr(), x_new.data_ptr(), status.data_ptr(), xa_per_profile=True,
                           d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(), d_post_var=post_var.data_ptr(), d_nobs=nobs.data_ptr(),
                           stream=cur())

    kt2, kh2 = k_t.reshape(nprof * m, nlev), k_h.reshape(nprof * m, nlev)
    held, per_rank = {}, {}
    paths, inner = [], {}
    for r in RANKS:
        sb = StateBasis.from_covariance(torch.tensor(sa_h), r)
        _, handle = sb.native_handle(nblk, 0)
        b = sb.b.to("cuda")
        q = dict(sb=sb, handle=handle, b=b, bt=b[:nlev].contiguous(), bh=b[nlev:].contiguous(), sa_c=sb.sa_c.to("cuda").contiguous(),
                 k_c=torch.empty((nprof, m, r), **f64), c=torch.zeros((nprof, 1, r), **f64), c_a=torch.zeros((1, r), **f64),
                 c_new=torch.empty((nprof, 1, r), **f64), pv=torch.empty((nprof, 1, r), **f64))
        per_rank[r] = q

        def project(q=q):
            ctx.basis_project_device(q["handle"], nprof, m, [k_t.data_ptr(), k_h.data_ptr()], q["k_c"].data_ptr(), stream=cur())

        def torch_product(q=q, r=r):
            held[r] = torch.matmul(kt2, q["bt"]) + torch.matmul(kh2, q["bh"])

        def reduced(q=q, r=r, project=project):
            k_matrix()
            project()
            ctx.oe_step_device(nprof, r, m, [q["k_c"].data_ptr()], q["c"].data_ptr(), q["c_a"].data_ptr(), q["sa_c"].data_ptr(),
                               se.data_ptr(), y.data_ptr(), fx.data_ptr(), q["c_new"].data_ptr(), status.data_ptr(),
                               d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(), d_post_var=q["pv"].data_ptr(), d_nobs=nobs.data_ptr(),
                               stream=cur())

        paths += [(f"project_r{r}", project), (f"torch_r{r}", torch_product), (f"reduced_r{r}", reduced)]
        inner[f"project_r{r}"] = inner[f"torch_r{r}"] = max(1, a.inner)
    paths.append(("full", full))
    for _ in range(3):
        for _, fn in paths:
            fn()                                               # warm-up: code objects, small copies, torch's allocator
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
           "calls_per_event_pair_project_and_torch": max(1, a.inner), "hbm_copy_tb_s": HBM_MEASURED_TB_S,
           "mfma_variant": "not built: plain fp64 FMA register tiles only, no A/B exists"}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    for r in RANKS:
        q = per_rank[r]
        paths[[nm for nm, _ in paths].index(f"project_r{r}")][1]()
        ref = torch.matmul(kt2, q["bt"]) + torch.matmul(kh2, q["bh"])
        torch.cuda.synchronize()
        scale = torch.matmul(kt2.abs(), q["bt"].abs()) + torch.matmul(kh2.abs(), q["bh"].abs())
        moved = 8.0 * nprof * m * (n + r) + 8.0 * n * r                  # K in once, K B out, B
        sec = res[f"project_r{r}"]["median_ms"] * 1e-3
        res[f"r{r}"] = {
            "bytes_moved": moved, "gb_s": moved / sec / 1e9, "share_of_copy_rate": moved / sec / (HBM_MEASURED_TB_S * 1e12),
            "fma": float(nprof) * m * n * r, "gfma_s": float(nprof) * m * n * r / sec / 1e9,
            "ratio_project_over_torch": res[f"project_r{r}"]["median_ms"] / res[f"torch_r{r}"]["median_ms"],
            "ratio_reduced_over_full": res[f"reduced_r{r}"]["median_ms"] / res["full"]["median_ms"],
            "largest_difference_project_vs_torch_of_n_u_sum_abs": float(
                ((q["k_c"].reshape(nprof * m, r) - ref).abs() / (n * 2.0 ** -53 * scale).clamp_min(1e-300)).max())}
        q["sb"].close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
