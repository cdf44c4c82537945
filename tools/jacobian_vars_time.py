"""Device time of the K-matrix in retrieval variables next to what it replaces, one process, one stream, HIP events, at
1000 profiles x 14 channels (HATPRO) x 7 elevations x 180 levels, R24:

  (a) raw        mwrt_tb_jacobian_batch_device (k_absorb_tl + k_jac_rte): rows in the operator's variables
  (b) variables  mwrt_tb_jacobian_batch_vars_device with ppmv + hydrostatic heights and d_dtb_ddz = NULL
  (c) raw+torch  (a) followed by the same change of variables written in torch on the device (what a caller did before)
  chain          the torch step of (c) alone

Every path is timed as a whole with one pair of HIP events on the current stream around it, after warm-up.
Usage: python tools/jacobian_vars_time.py [--reps N] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr


def goff_gratch_es(t):
    y = 373.16 / t
    g = (-7.90298 * (y - 1.0) + 5.02808 * torch.log10(y) - 1.3816e-07 * (10.0 ** (11.344 * (1.0 - 1.0 / y)) - 1.0)
         + 0.0081328 * (10.0 ** (-3.49149 * (y - 1.0)) - 1.0) + float(np.log10(1013.246)))
    return 10.0 ** g


def torch_chain(a_t, a_e, zr, p, t, rh):
    """ppmv + hydrostatic heights from the raw rows [nprof][nang][nf][nlev] and the level arrays [nprof][nlev]."""
    e = rh * goff_gratch_es(t)
    c = torch.zeros_like(p)
    c[:, 1:] = 287.04 / (2.0 * 9.80665) * torch.log(p[:, :-1] / p[:, 1:]) / 1000.0
    lo = zr * c[:, None, None, :]
    g = lo.clone()
    g[..., :-1] += lo[..., 1:]
    ipe = 1.0 / (p - 0.378 * e)
    k_t = 1.0 + 0.608 * (0.622 * e * ipe)
    k_e = 0.608 * t * 0.622 * p * ipe * ipe
    d_t = a_t + g * k_t[:, None, None, :]
    d_q = (a_e + g * k_e[:, None, None, :]) * (p / 1e6)[:, None, None, :]
    return d_t, d_q


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
    out = [torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(2)]
    valid = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    variables = nat.JacVariables.of(humidity="ppmv", heights="hydrostatic")
    cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    lev = (z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr())

    def raw():
        ctx.tb_jacobian_batch_device("R24", nprof, nlev, *lev, frq, ang, tb.data_ptr(), *[j.data_ptr() for j in jac],
                                     valid.data_ptr(), stream=cur())

    def with_variables():
        ctx.tb_jacobian_batch_vars_device("R24", nprof, nlev, *lev, frq, ang, tb.data_ptr(), out[0].data_ptr(),
                                          out[1].data_ptr(), valid.data_ptr(), variables=variables, stream=cur())

    def chain():
        return torch_chain(jac[0], jac[1], jac[2], p, t, rh)

    def raw_then_torch():
        raw()
        return chain()
    res = {"shape": {"nprof": nprof, "nf": nf, "nang": nang, "nlev": nlev, "model": "R24"}, "reps": a.reps}
    for name, fn in (("raw", raw), ("variables", with_variables), ("raw_then_torch", raw_then_torch), ("torch_chain", chain)):
        for _ in range(3):
            fn()                                           # warm-up: workspace, small copies, code objects, torch's allocator
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        res[name] = {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)),
                     "p90_ms": float(np.percentile(ms, 90)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    # the two routes give the same rows
    with_variables()
    d_t, d_q = raw_then_torch()
    torch.cuda.synchronize()
    res["largest_difference_of_a_row"] = {
        "dtb_dt": float(((out[0] - d_t).abs().amax(-1) / d_t.abs().amax(-1)).max()),
        "dtb_dppmv": float(((out[1] - d_q).abs().amax(-1) / d_q.abs().amax(-1)).max())}
    res["ratio_variables_over_raw"] = res["variables"]["median_ms"] / res["raw"]["median_ms"]
    res["ratio_variables_over_raw_then_torch"] = res["variables"]["median_ms"] / res["raw_then_torch"]["median_ms"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
