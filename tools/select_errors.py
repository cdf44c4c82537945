"""Largest error of every output of mwrt_oe_select_device against the longdouble reference (tests/select_reference.py), over
the shapes and the two variance variants tests/test_oe_select.py runs (driven through tests/select_device.py, which that
test uses too), in units of that test's bars (1.0 is the bar): the numbers DESIGN.md 4.12 records.  Per shape the maxima over
the variants and the profiles, and the smallest margin (best - runner-up) / best of any round; ``worst`` holds the largest of
each output over all shapes.  Every profile's order is asserted to be the reference's greedy order on the way.
Usage: python tools/select_errors.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import select_device as sd
import select_reference as sr
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    res = {"units": {"q_pick": "64 (n + nsel) eps b_j, b_i = |k_i|^T |S0| |k_i| / se_i", "q": "64 (n + nsel) eps b_i",
                     "dfs_gain": "64 (n + nsel) eps |v|^T |Sa^-1| |v| / d", "post_cov": "64 (n + nsel) eps max |S0|",
                     "post_var": "as post_cov"},
           "bar": 1.0, "min_margin_required": sr.MIN_MARGIN, "shapes": {}}
    worst = {}
    for nlev, nblk, m, nsel in sr.SHAPES:
        row = {"min_margin": float("inf")}
        for se_pp in (False, True):
            case, greedy = sr.seeded(nlev, nblk, m, nsel, se_pp)
            got = sd.SelDev(case, nsel).select(ctx)
            for key, v in sd.judge(case, got, greedy, nsel, label=(nlev, nblk, m, nsel, se_pp)).items():
                row[key] = max(row.get(key, 0.0), v)
            row["min_margin"] = min(row["min_margin"], float(min(np.nanmin(r["margin"]) for r in greedy)))
        res["shapes"][f"{nlev}-{nblk}-{m}-{nsel}"] = row
        for key, v in row.items():
            worst[key] = min(worst.get(key, v), v) if key == "min_margin" else max(worst.get(key, 0.0), v)
    res["worst"] = worst
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
