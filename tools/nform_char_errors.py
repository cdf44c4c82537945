"""Largest error of every output of mwrt_oe_nform_char_device and mwrt_oe_nform_gain_device against the NumPy reference
(tests/nform_char_reference.py), over the shapes and the four (se, xa) variants tests/test_oe_nform_char.py runs (driven
through tests/nform_char_device.py, which that test uses too), in the units of that test's bar: the numbers DESIGN.md 4.11.1
records.  Per shape the maxima over the variants and the profiles; ``worst`` holds the largest of each output over all shapes,
``bar`` what the test holds them to.  Usage: python tools/nform_char_errors.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import nform_char_device as tc
import nform_char_reference as ncr
import nform_reference as nfr
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    res = {"units": {"gain": "max |ref| per (profile, block)", "avk": "max of |S^| |H| over the sub-block", "avk_diag": "as avk",
                     "dfs_block": "max(1, sum of the block's diagonal of |S^| |H|)", "noise_var": "sqrt(max diag Sa of block j * of block k)",
                     "smooth_var": "as noise_var", "post_cov": "as noise_var", "gain_from_solve": "as gain, S^ and status from the solve entry"},
           "bar": nfr.TOL, "shapes": {}}
    worst = {}
    for nlev, nblk, m in ncr.SHAPES:
        row = {"cond_jacobi_scaled_max": 0.0}
        for se_pp, xa_pp in ((False, False), (True, False), (False, True), (True, True)):
            case, ref = tc.seeded(nlev, nblk, m, se_pp, xa_pp, 4)
            d = tc.CharDev(case)
            got = d.characterise(ctx)
            err = ncr.char_errors(tc.as_reference(got), ref, case)
            ctx.oe_nform_solve_device(**d.solve_args())
            ctx.oe_nform_gain_device(**d.gain_args(from_solve=True))
            torch.cuda.synchronize()
            err["gain_from_solve"] = ncr.char_errors(dict(gain=d.host()["gain"]), ref, case)["gain"]
            for key, v in err.items():
                row[key] = max(row.get(key, 0.0), v)
            row["cond_jacobi_scaled_max"] = max(row["cond_jacobi_scaled_max"], float(np.nanmax(ref["cond"])))
        res["shapes"][f"{nlev}-{nblk}-{m}"] = row
        for key, v in row.items():
            worst[key] = max(worst.get(key, 0.0), v)
    res["worst"] = worst
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
