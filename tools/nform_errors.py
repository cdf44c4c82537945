"""Largest error of every output of mwrt_oe_nform_prepare_device, mwrt_oe_nform_solve_device and mwrt_oe_nform_cost_device
against the NumPy reference (tests/nform_reference.py), over the shapes and the four (se, xa) variants tests/test_oe_nform.py
runs (driven through tests/nform_device.py, which that test uses too), in the units of that test's bars: the numbers DESIGN.md 4.11 records.  Per shape the maxima over the variants and the
profiles; ``worst`` holds the largest of each output over all shapes, ``bars`` what the tests hold them to.
Usage: python tools/nform_errors.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import nform_reference as nfr
import nform_device as tn
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    eps = np.finfo(np.float64).eps
    res = {"units": {"x_new": "max |x_ref - xa| per block", "post_var": "max diag Sa per block", "post_cov": "max |C^-1|",
                     "dfs": "max(1, |ref|)", "chi2": "max(1, d^T W d)", "h": "max diag H", "g": "sum_i |K_ij w_i r_i|", "rwr": "|ref|",
                     "cost": "sum_kept r^2 / se + |dx|^T |Sa^-1| |dx|", "x_new_damped": "as x_new, gamma = (0, 0.5, 1e3, 0)"},
           "bars": {"solve": nfr.TOL, "prepare": "64 m eps", "cost": "64 (m + n) eps"}, "shapes": {}}
    worst = {}
    for nlev, nblk, m in nfr.SHAPES:
        n = nlev * nblk
        row = {"cond_jacobi_scaled_max": 0.0, "prepare_bar": 64 * m * eps, "cost_bar": 64 * (m + n) * eps}
        for se_pp, xa_pp in ((False, False), (True, False), (False, True), (True, True)):
            case, gamma, (lin, sol, cost), (_, damped, _) = tn.seeded(nlev, nblk, m, se_pp, xa_pp, 4)
            d = tn.Dev(case)
            got = d.run(ctx)
            d.reset()
            again = d.run(ctx, gamma=gamma)
            err = dict(nfr.prepare_errors(got, lin), **nfr.solve_errors({k: got[k] for k in ("x_new", "chi2", "dfs", "post_var", "post_cov")}, sol, case))
            err["x_new_damped"] = nfr.solve_errors(dict(x_new=again["x_new"]), damped, case)["x_new"]
            err["cost"] = float((np.abs(got["cost"] - cost["cost"]) / cost["scale"]).max())
            for key, v in err.items():
                row[key] = max(row.get(key, 0.0), v)
            row["cond_jacobi_scaled_max"] = max(row["cond_jacobi_scaled_max"], float(np.nanmax(sol["cond"])), float(np.nanmax(damped["cond"])))
        res["shapes"][f"{nlev}-{nblk}-{m}"] = row
        for key, v in row.items():
            worst[key] = max(worst.get(key, 0.0), v)
    torch.cuda.synchronize()
    res["worst"] = worst
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
