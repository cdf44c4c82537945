"""Largest error of every output of mwrt_oe_step_device against the NumPy reference (tests/oe_reference.py), over the shapes
and variants tests/test_oe_step.py runs, in the units of that test's bars (x_new of max |x_ref - xa| per block, post_var of
max diag Sa per block, chi2 and dfs of max(1, |ref|)); the bar itself is 1e-8.
Usage: python tools/oe_step_errors.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def run(ctx, case):
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")   # noqa: E731
    k = [dev(b) for b in case["k"]]
    nprof, m, nlev = k[0].shape
    x, xa, sa, se, y, fx = (dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(x_new=torch.empty_like(x), post_var=torch.empty_like(x), chi2=torch.empty(nprof, **f64),
               dfs=torch.empty(nprof, **f64), nobs=torch.empty(nprof, dtype=torch.int32, device="cuda"),
               status=torch.empty(nprof, dtype=torch.uint8, device="cuda"))
    ctx.oe_step_device(nprof, nlev, m, [b.data_ptr() for b in k], x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(),
                       y.data_ptr(), fx.data_ptr(), out["x_new"].data_ptr(), out["status"].data_ptr(),
                       d_chi2=out["chi2"].data_ptr(), d_dfs=out["dfs"].data_ptr(), d_post_var=out["post_var"].data_ptr(),
                       d_nobs=out["nobs"].data_ptr(), xa_per_profile=case["xa"].ndim == 3, se_full=case["se"].ndim == 2,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.Context(0)
    res = {"bar": oer.TOL, "cases": {}, "max": {k: 0.0 for k in ("x_new", "post_var", "chi2", "dfs")}, "max_cond": 0.0}
    for nlev, nblk, m in oer.SHAPES:
        for se_full in (False, True):
            for xa_pp in (False, True):
                case = oer.make_case(nlev, nblk, m, nprof=3 if nlev >= 180 else 4, se_full=se_full, xa_per_profile=xa_pp)
                ref = oer.oe_step_reference(**case)
                got = run(ctx, case)
                err = oer.block_errors(got, ref, case)
                err["cond"] = float(np.nanmax(ref["cond"]))
                res["cases"][f"{nlev}-{nblk}-{m}-{'full' if se_full else 'diag'}-{'perprofile' if xa_pp else 'shared'}"] = err
                for k in res["max"]:
                    res["max"][k] = max(res["max"][k], err[k])
                res["max_cond"] = max(res["max_cond"], err["cond"])
    txt = json.dumps(res, indent=1)
    print(json.dumps({"max": res["max"], "max_cond": res["max_cond"]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
