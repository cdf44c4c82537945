"""Device time of the ray-traced K-matrix next to the plane-parallel one from the same build, one process, one stream, HIP
events (mwrt_set_timing), the paths run alternately, at 1000 profiles x 14 channels (HATPRO) x 7 elevations x 180 levels, R24:
  (a) mwrt_tb_jacobian_batch_ray_device (k_ray_paths_tl + k_absorb_tl + k_jac_rte_ray), clear sky, raw rows
  (b) mwrt_tb_jacobian_batch_vars_device (k_absorb_tl + k_jac_rte), the same call
  (c), (d) the two with cloud liquid and ice and the variables (ppmv, kg/kg, hydrostatic)
and the launches of (a) one by one (events around each: the path kernel, the absorption, the adjoint RTE).
Usage: python tools/ray_jacobian_time.py [--reps N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr, spectroscopy as sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    ctx = nat.Context(0)
    m = sp.get_model("R24")
    nprof, nlev, frq, ang = a.nprof, pr.N_LEVELS, pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
    nf, nang = frq.size, ang.size
    P = pr.synthetic_profiles(nprof, 2)
    f64 = dict(dtype=torch.float64, device="cuda")
    z, p, t, rh = (torch.tensor(P[k], **f64) for k in ("z", "p", "t", "rh"))
    h = z - z[:, :1]
    denliq = torch.where((h > 1.0) & (h < 2.0), torch.full_like(h, 0.2), torch.zeros_like(h))
    denice = torch.where((h > 6.0) & (h < 7.0), torch.full_like(h, 0.05), torch.zeros_like(h))
    tb = torch.empty((nprof, nang, nf), **f64)
    jac = [torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(5)]
    valid = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    prof = (z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr())
    cloud = dict(d_denliq=denliq.data_ptr(), d_denice=denice.data_ptr(), d_dtb_dliq=jac[3].data_ptr(),
                 d_dtb_dice=jac[4].data_ptr(), variables=nat.JacVariables(2, 1, 1, 0))

    def call(entry, **kw):
        return lambda: entry(m, nprof, nlev, *prof, frq, ang, tb.data_ptr(), jac[0].data_ptr(), jac[1].data_ptr(),
                             valid.data_ptr(), d_dtb_ddz=jac[2].data_ptr(), **kw)
    calls = {
        "a_ray_clear": call(ctx.tb_jacobian_batch_ray_device),
        "b_vars_clear": call(ctx.tb_jacobian_batch_vars_device),
        "c_ray_cloudy_ppmv_kgkg_hydrostatic": call(ctx.tb_jacobian_batch_ray_device, **cloud),
        "d_vars_cloudy_ppmv_kgkg_hydrostatic": call(ctx.tb_jacobian_batch_vars_device, **cloud),
    }
    for fn in calls.values():
        for _ in range(3):
            fn()                                       # warm-up: workspaces, device copies, code objects
    ctx.synchronize()
    ms = {k: [] for k in calls}
    launches = {}
    for _ in range(a.reps):                            # the paths alternate: a drift of the clocks reaches all alike
        for name, fn in calls.items():
            ctx.set_timing(True)
            fn()
            total, n = ctx.timing_collect()            # device time of the call's launches (HIP events on the stream)
            ms[name].append(total)
            launches[name] = n
    ctx.set_timing(False)
    res = {"shape": {"nprof": nprof, "nf": nf, "nang": nang, "nlev": nlev, "model": "R24"}, "reps": a.reps}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
                     "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "launches": launches[name]}
    med = lambda k: res[k]["median_ms"]   # noqa: E731
    res["ratio_a_over_b"] = med("a_ray_clear") / med("b_vars_clear")
    res["ratio_c_over_d"] = med("c_ray_cloudy_ppmv_kgkg_hydrostatic") / med("d_vars_cloudy_ppmv_kgkg_hydrostatic")
    # the kernels separately: the adjoint RTE is each call's last launch (mwrt_last_kernel_ms); k_absorb_tl is what is left of
    # (b), which has two launches; the path kernel is what is then left of (a), which has three
    rte = {}
    for name in ("a_ray_clear", "b_vars_clear"):
        v = []
        for _ in range(a.reps):
            ctx.set_timing(True)
            calls[name]()
            v.append(ctx.last_kernel_ms())
            ctx.timing_collect()
        rte[name] = float(np.median(v))
    ctx.set_timing(False)
    absorb = med("b_vars_clear") - rte["b_vars_clear"]
    res["kernels_ms"] = {"k_jac_rte_ray": rte["a_ray_clear"], "k_jac_rte": rte["b_vars_clear"], "k_absorb_tl": absorb,
                         "k_ray_paths_tl": med("a_ray_clear") - rte["a_ray_clear"] - absorb}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
