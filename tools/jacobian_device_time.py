"""Device time of the device K-matrix path next to the forward call, one process, one stream, HIP events
(mwrt_set_timing): mwrt_tb_jacobian_batch_device (k_absorb_tl + k_jac_rte), mwrt_tb_jacobian_batch_opt_device with a cloud in
every profile (skipped on a library without it), mwrt_absorption_tl_batch_device (k_absorb_tl
alone) and mwrt_tb_batch_device (the fused forward kernel), at 1000 profiles x 14 channels (HATPRO) x 7 elevations x 180
levels, R24.  Usage: python tools/jacobian_device_time.py [--reps N] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    P = pr.synthetic_profiles(nprof, 2)
    z, p, t, rh = (torch.tensor(P[k], dtype=torch.float64, device="cuda") for k in ("z", "p", "t", "rh"))
    f64 = dict(dtype=torch.float64, device="cuda")
    tb = torch.empty((nprof, nang, nf), **f64)
    jac = [torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(3)]
    absn = [torch.empty((nprof, nf, nlev), **f64) for _ in range(6)]
    valid = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    # a cloud in every profile: liquid over levels 20-39, ice over levels 60-79
    cloud = np.zeros((2, nprof, nlev))
    cloud[0, :, 20:40] = np.linspace(0.1, 0.3, 20)
    cloud[1, :, 60:80] = np.linspace(0.02, 0.08, 20)
    denl, deni = (torch.tensor(c, **f64) for c in cloud)
    cjac = [torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(2)]
    torch.cuda.synchronize()
    calls = {
        "tb_jacobian_batch_device": lambda: ctx.tb_jacobian_batch_device(
            "R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb.data_ptr(),
            *[j.data_ptr() for j in jac], valid.data_ptr()),
        "tb_jacobian_batch_opt_device_cloudy": lambda: ctx.tb_jacobian_batch_opt_device(
            "R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb.data_ptr(),
            *[j.data_ptr() for j in jac], valid.data_ptr(), d_denliq=denl.data_ptr(), d_denice=deni.data_ptr(),
            d_dtb_dliq=cjac[0].data_ptr(), d_dtb_dice=cjac[1].data_ptr()),
        "absorption_tl_batch_device": lambda: ctx.absorption_tl_batch_device(
            "R24", nprof, nlev, p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, *[x.data_ptr() for x in absn]),
        "tb_batch_device": lambda: ctx.tb_batch_device(
            "R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb.data_ptr(),
            valid.data_ptr()),
    }
    res = {"shape": {"nprof": nprof, "nf": nf, "nang": nang, "nlev": nlev, "model": "R24"}, "reps": a.reps}
    if not hasattr(ctx._lib, "mwrt_tb_jacobian_batch_opt_device") or "mwrt_tb_jacobian_batch_opt_device" not in nat.SIGNATURES:
        del calls["tb_jacobian_batch_opt_device_cloudy"]
    for name, fn in calls.items():
        for _ in range(3):
            fn()                                       # warm-up: workspace, frequency / air-mass copies, code objects
        ctx.synchronize()
        ms = []
        for _ in range(a.reps):
            ctx.set_timing(True)
            fn()
            total, launches = ctx.timing_collect()     # device time of the call's launches (HIP events on the stream)
            ms.append(total)
        ctx.set_timing(False)
        ms = np.array(ms)
        res[name] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                     "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "launches": launches}
    if "tb_jacobian_batch_opt_device_cloudy" in res:
        res["ratio_cloudy_jacobian_over_clear"] = (res["tb_jacobian_batch_opt_device_cloudy"]["median_ms"]
                                                   / res["tb_jacobian_batch_device"]["median_ms"])
    res["ratio_jacobian_over_forward"] = res["tb_jacobian_batch_device"]["median_ms"] / res["tb_batch_device"]["median_ms"]
    res["ratio_tl_absorption_over_forward"] = res["absorption_tl_batch_device"]["median_ms"] / res["tb_batch_device"]["median_ms"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
