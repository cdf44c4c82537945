"""Device time of the spectroscopic-parameter Jacobian next to the K-matrix call and to what it replaces, one process, one
stream, HIP events (mwrt_set_timing), the paths run alternately, at 1000 profiles x 14 channels (HATPRO) x 7 elevations x 180
levels, R24, 30 parameters mixing per-line, scalar and [*] ones:
  (a) mwrt_tb_param_jacobian_batch_device (k_absorb_tl + k_par_tangent + k_par_contract); also with the per-line parameters
      alone and with the full-sum parameters (o2_x and the [*] ones) alone, which says where its time goes
  (b) mwrt_tb_jacobian_batch_device (k_absorb_tl + k_jac_rte)
  (c) central differences as a user forms them without it: 2 npar mwrt_tb_batch_device calls on pre-registered perturbed models
Usage: python tools/param_jacobian_time.py [--reps N] [--out FILE.json]"""
import argparse
import copy
import dataclasses
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr, sensitivity, spectroscopy as sp

SPECS = ["h2o_cf", "h2o_cs", "h2o_xcf", "h2o_xcs", "o2_x", "o2_wb300", "n2_l",
         "h2o_s1[0]", "h2o_b2[0]", "h2o_w0[0]", "h2o_x[0]", "h2o_w0s[0]", "h2o_xs[0]", "h2o_sh[0]", "h2o_shs[0]",
         "o2_s300[1]", "o2_be[1]", "o2_w300[1]", "o2_y0[1]", "o2_y1[1]", "o2_g0[1]", "o2_g1[1]", "o2_dnu0[1]", "o2_dnu1[1]",
         "o2_w300[5]", "o2_y0[9]", "h2o_w0[*]", "o2_w300[*]", "o2_y0[*]", "o2_s300[*]"]


def perturbed(m, q, factor):
    if q.field < nat.PAR_FIRST_H2O_LINE_FIELD:
        return dataclasses.replace(m, **{q.name: q.value * factor})
    species, key = q.name.split("_", 1)
    h2o, o2 = copy.deepcopy(m.h2o), copy.deepcopy(m.o2)
    col = (h2o if species == "h2o" else o2)[key]
    if q.line < 0:
        col *= factor
    else:
        col[q.line] *= factor
    return dataclasses.replace(m, h2o=h2o, o2=o2)


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
    recs = sensitivity.parse_params(m, SPECS)
    full = [q for q in recs if q.line < 0 or q.name == "o2_x"]
    lines = [q for q in recs if q not in full]
    P = pr.synthetic_profiles(nprof, 2)
    z, p, t, rh = (torch.tensor(P[k], dtype=torch.float64, device="cuda") for k in ("z", "p", "t", "rh"))
    f64 = dict(dtype=torch.float64, device="cuda")
    tb = torch.empty((nprof, nang, nf), **f64)
    kb = torch.empty((nprof, nang, nf, len(recs)), **f64)
    jac = [torch.empty((nprof, nang, nf, nlev), **f64) for _ in range(3)]
    valid = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    models = [perturbed(m, q, 1.0 + s * 1e-4) for q in recs for s in (1, -1)]
    prof = (z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr())

    def par(which):
        return lambda: ctx.tb_param_jacobian_device(m, nprof, nlev, *prof, frq, ang, [(q.field, q.line) for q in which],
                                                    kb.data_ptr(), valid.data_ptr(), d_tb=tb.data_ptr())

    def differences():
        for tab in models:
            ctx.tb_batch_device(tab, nprof, nlev, *prof, frq, ang, tb.data_ptr(), valid.data_ptr())
    calls = {
        "a_param_jacobian": par(recs),
        "a_per_line_and_closed_form_only": par(lines),
        "a_full_sum_only": par(full),
        "b_tb_jacobian_batch_device": lambda: ctx.tb_jacobian_batch_device(m, nprof, nlev, *prof, frq, ang, tb.data_ptr(),
                                                                           *[j.data_ptr() for j in jac], valid.data_ptr()),
        "c_central_differences_2npar_forward_calls": differences,
        "tb_batch_device": lambda: ctx.tb_batch_device(m, nprof, nlev, *prof, frq, ang, tb.data_ptr(), valid.data_ptr()),
    }
    for fn in calls.values():
        for _ in range(3):
            fn()                                       # warm-up: workspaces, device copies, model uploads, code objects
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
    res = {"shape": {"nprof": nprof, "nf": nf, "nang": nang, "nlev": nlev, "model": "R24"}, "reps": a.reps,
           "npar": {"a_param_jacobian": len(recs), "a_per_line_and_closed_form_only": len(lines), "a_full_sum_only": len(full)},
           "params": SPECS}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
                     "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "launches": launches[name]}
    med = lambda k: res[k]["median_ms"]   # noqa: E731
    res["ratio_a_over_b"] = med("a_param_jacobian") / med("b_tb_jacobian_batch_device")
    res["ratio_c_over_a"] = med("c_central_differences_2npar_forward_calls") / med("a_param_jacobian")
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
