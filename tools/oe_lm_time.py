"""Device time of the Levenberg-Marquardt split of the optimal-estimation step (mwrt_oe_lm_prepare_device,
mwrt_oe_lm_solve_device, mwrt_oe_cost_device) next to the unsplit step, one process, one stream, HIP events,
at 1000 profiles x 180 levels x 2 blocks (T, rh) x 98 observations (14 channels x 7 elevations), K from the device
K-matrix call on the synthetic profiles:

  prepare     mwrt_oe_lm_prepare_device: the row rule, r, K dx and G0 = K Sa K^T
  solve       mwrt_oe_lm_solve_device: one damped trial on that linearisation (gamma = 1)
  cost        mwrt_oe_cost_device: J at a state
  oe_x_only   (a) mwrt_oe_step_device, x_new and status only: the unsplit step
  k_matrix    the mwrt_tb_jacobian_batch_vars_device call that produces K -- and the forward run OneDVar.forward makes
  tb_only     mwrt_tb_batch_device at the same state, TBs alone: what a forward run costs without the Jacobian

The paths are run alternately, repetition by repetition, each between one pair of HIP events on the current stream.  The
point of the split is the price of a rejected trial against a fresh step; both ratios are reported whichever way they come
out: rejected trial (solve + forward run + cost) over fresh step ((a) + k_matrix), with the forward run as retrieve_lm
makes it (k_matrix) and as the TB-only entry would make it, and prepare + solve over (a).
Usage: python tools/oe_lm_time.py [--reps N] [--nprof N] [--out FILE.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oe_lm_time.json"))
    a = ap.parse_args()
    ctx = nat.Context(0)
    nprof, nlev, frq, ang = a.nprof, pr.N_LEVELS, pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
    nf, nang = frq.size, ang.size
    m, nblk = nf * nang, 2
    n = nblk * nlev
    f64 = dict(dtype=torch.float64, device="cuda")
    u8 = dict(dtype=torch.uint8, device="cuda")
    P = pr.synthetic_profiles(nprof, 2)
    z, p, t, rh = (torch.tensor(P[k], **f64) for k in ("z", "p", "t", "rh"))
    tb, tb2 = torch.empty((nprof, nang, nf), **f64), torch.empty((nprof, nang, nf), **f64)
    k_t, k_h = (torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(2))
    valid = torch.empty(nprof, **u8)
    variables = nat.JacVariables.of(humidity="rh")
    cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

    def k_matrix():
        ctx.tb_jacobian_batch_vars_device("R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang,
                                          tb.data_ptr(), k_t.data_ptr(), k_h.data_ptr(), valid.data_ptr(), variables=variables,
                                          stream=cur())

    def tb_only():
        ctx.tb_batch_device("R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb2.data_ptr(),
                            valid.data_ptr(), stream=cur())

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
    inv = np.linalg.inv(sa_h)
    sa_inv = torch.tensor(0.5 * (inv + inv.T), **f64)
    x = torch.stack([t, rh], dim=1).contiguous()
    xa = (x + torch.tensor(rng.standard_normal((nprof, nblk, nlev)) * np.array([0.5, 0.02])[None, :, None], **f64)).contiguous()
    fx = tb.reshape(nprof, m)
    y = fx + torch.tensor(rng.standard_normal((nprof, m)) * 0.5, **f64)
    gamma = torch.ones(nprof, **f64)
    g0, r, kdx = torch.empty((nprof, m * (m + 1) // 2), **f64), torch.empty((nprof, m), **f64), torch.empty((nprof, m), **f64)
    keep, lin_status, status = torch.empty((nprof, m), **u8), torch.empty(nprof, **u8), torch.empty(nprof, **u8)
    x_new, x_step, cost = torch.empty_like(x), torch.empty_like(x), torch.empty(nprof, **f64)
    kp = [k_t.data_ptr(), k_h.data_ptr()]
    lin = dict(d_g0=g0.data_ptr(), d_r=r.data_ptr(), d_kdx=kdx.data_ptr(), d_keep=keep.data_ptr(), d_lin_status=lin_status.data_ptr())

    def prepare():
        ctx.oe_lm_prepare_device(nprof, nlev, m, kp, x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(), y.data_ptr(),
                                 fx.data_ptr(), xa_per_profile=True, stream=cur(), **lin)

    def solve():
        ctx.oe_lm_solve_device(nprof, nlev, m, kp, x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(), gamma.data_ptr(),
                               d_x_new=x_new.data_ptr(), d_status=status.data_ptr(), xa_per_profile=True, stream=cur(), **lin)

    def cost_call():
        ctx.oe_cost_device(nprof, nlev, m, nblk, x.data_ptr(), xa.data_ptr(), se.data_ptr(), y.data_ptr(), fx.data_ptr(),
                           keep.data_ptr(), sa_inv.data_ptr(), cost.data_ptr(), xa_per_profile=True, stream=cur())

    def oe():
        ctx.oe_step_device(nprof, nlev, m, kp, x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(), y.data_ptr(),
                           fx.data_ptr(), x_step.data_ptr(), status.data_ptr(), xa_per_profile=True, stream=cur())

    paths = (("prepare", prepare), ("solve", solve), ("cost", cost_call), ("oe_x_only", oe), ("k_matrix", k_matrix),
             ("tb_only", tb_only))
    for _ in range(3):
        for _, fn in paths:
            fn()                                               # warm-up: code objects, LDS limits, small copies
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
    res = {"shape": {"nprof": nprof, "nlev": nlev, "nblk": nblk, "m": m, "model": "R24"}, "reps": a.reps}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    med = {name: res[name]["median_ms"] for name, _ in paths}
    fresh = med["oe_x_only"] + med["k_matrix"]
    res["rejected_trial_over_fresh_step"] = (med["solve"] + med["k_matrix"] + med["cost"]) / fresh
    res["rejected_trial_with_tb_only_forward_over_fresh_step"] = (med["solve"] + med["tb_only"] + med["cost"]) / fresh
    res["prepare_plus_solve_over_oe_x_only"] = (med["prepare"] + med["solve"]) / med["oe_x_only"]
    # the split computes what the step computes: gamma = 0 on the linearisation against (a)
    gamma.zero_()
    prepare()
    solve()
    oe()
    torch.cuda.synchronize()
    scale = (x_step - xa).abs().amax(dim=2, keepdim=True)
    res["largest_difference_split_at_gamma_0_vs_step_of_block_scale"] = float(((x_new - x_step).abs() / scale).max())
    res["tb_only_vs_k_matrix_tb_max_abs_K"] = float((tb2 - tb).abs().max())
    res["status_counts"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
