"""Measured error of the two K2 kernels on the hand-built columns of tests/rte_cases.py, against the long-double reference of
tests/rte_reference.py and under the bars derived there: per case and entry the device's error, the error of the double oracle
(oracle/lbl_oracle.py planck_down + bright on the same columns) and the bar, plus the bit-for-bit properties
tests/test_rte_columns.py asserts.  error / bar <= 1 passes.
Usage: python tools/rte_column_errors.py [--out profiles/rte_column_errors.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import rte_cases as rc
import rte_device as rd
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    res = {"units": "kelvin: max_abs_K = largest |TB - reference|; bar_K_*: the derived absolute bar (smallest, largest, at the worst point); "
                    "worst_err_over_bar: largest error / bar over every output of the case; nan_by_contract: outputs asserted NaN and left out",
           "reference": "tests/rte_reference.py, np.longdouble (held to mpmath at 50 digits by tests/test_rte_reference.py)",
           "entries": {"tau": "k_rte_tau through mwrt_tb_from_layer_tau_device", "alpha": "K2 of k_tb_fused through mwrt_tb_from_absorption_device"},
           "device": {"tau": {}, "alpha": {}}, "oracle": {"tau": {}, "alpha": {}}, "exact": {}}
    for name in rc.names(held=True):
        case = rc.table()[name]
        tb, valid = rd.cached_run(ctx, name)
        rd.check_case(name, tb, valid, res["device"][case.entry])
        rd.check_case(name, rd.oracle_tb(case), case.valid_expected, res["oracle"][case.entry], label=name)
    for label, na, ia, nb, ib in rc.exact_pairs():
        x, y = rd.cached_run(ctx, na)[0][ia], rd.cached_run(ctx, nb)[0][ib]
        res["exact"][label] = dict(values=int(x.size), differing=int((np.ascontiguousarray(x).view(np.uint64) != np.ascontiguousarray(y).view(np.uint64)).sum()))
    for who in ("device", "oracle"):
        for entry in ("tau", "alpha"):
            rows = res[who][entry].values()
            res["worst_%s_%s" % (who, entry)] = dict(worst_err_over_bar=max(r["worst_err_over_bar"] for r in rows), max_abs_K=max(r["max_abs_K"] for r in rows))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
