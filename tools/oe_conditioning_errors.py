"""The error of the optimal-estimation solves up the conditioning ladder of tests/oe_exact_reference.py: per case and profile
cond_2 of what is factored, the error of the NumPy float64 reference (the yardstick) and of the device against the 50-digit
reference in the family's own units, both in units of eps cond, the bar, and per family the pooled constants c_out and the
worst device-to-bar and device-to-yardstick ratios: the numbers DESIGN.md 4.6, 4.10 and 4.11 record.  Driven through
tests/oe_conditioning_device.py, which tests/test_oe_conditioning.py uses too.
Usage: python tools/oe_conditioning_errors.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

import oe_conditioning_device as ocd
import oe_exact_reference as ex
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    res = {"bar": "max(8 c_out eps cond, 64 (m + n) eps); c_out = max over the family's cases of yardstick error / (eps cond)",
           "units": {"mform": "oe_reference.block_errors; gain outputs: oe_char_reference.char_errors",
                     "nform": "nform_reference.solve_errors (chi2 of max(1, d^T W d))",
                     "whiten": "l of max |L|; y, fx, k: whiten_reference.column_errors; the larger of the combined and the apply entry"},
           "digits": ex.DIGITS, "families": {}}
    for family, (cases, entry) in ex.FAMILIES.items():
        pooled = ex.pooled(family)
        fam = {"pooled_c": {k: float(v) for k, v in pooled.items()}, "cases": {}, "worst_device_over_bar": {},
               "worst_device_in_eps_cond": {}, "worst_device_over_yardstick_c": {}}
        for key in cases():
            e = entry(key)
            err, got = ocd.DEVICE_ERRORS[family](ctx, key)
            rows = []
            for i in range(ex.NPROF):
                unit = ex.EPS * float(e["cond"][i])
                row = {"cond": float(e["cond"][i]), "outputs": {}}
                for out, dev in err[i].items():
                    bar = ex.bar(family, key, out, i)
                    row["outputs"][out] = {"yardstick": e["err"][i][out], "device": dev, "yardstick_eps_cond": e["err"][i][out] / unit,
                                           "device_eps_cond": dev / unit, "bar": bar}
                    for name, v in (("worst_device_over_bar", dev / bar), ("worst_device_in_eps_cond", dev / unit),
                                    ("worst_device_over_yardstick_c", dev / unit / pooled[out])):
                        fam[name][out] = max(fam[name].get(out, 0.0), v)
                rows.append(row)
            fam["cases"][ex.case_id(key)] = {"status": [int(s) for s in got["status"]], "profiles": rows}
        res["families"][family] = fam
    torch.cuda.synchronize()
    txt = json.dumps(res, indent=1)
    print(json.dumps({f: {k: v for k, v in d.items() if k != "cases"} for f, d in res["families"].items()}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
