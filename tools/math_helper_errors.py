"""Measured error of every device arithmetic helper against the 50-digit references of tests/math_reference.py, on the
inputs tests/test_math_helpers.py uses and through the same functions (tests/math_helpers_device.py): per helper the number
of points, the largest relative and ulp error, the bar in the same units, where the bar comes from and the largest
error / bar ratio (<= 1 passes).  The collectives are bit-identical to their order emulations or the tests fail; for them
only block_suffix_excl's relative accuracy on terms falling from 1 to 1e-300 is a measured figure.
Usage: python tools/math_helper_errors.py [--out profiles/math_helper_errors.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import math_helpers_device as mh
import math_reference as mr
from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    res = {"units": "max_rel: |device - reference| / |reference| (complex results: moduli); max_ulp: in spacings of doubles at the reference; "
                    "bar_*: the bar in the same units at the point where it is widest; worst_err_over_bar: largest error / bar over the points",
           "reference": "tests/math_reference.py, decimal at %d digits" % mr.PREC, "helpers": {}}
    for name, fn in mh.CHECKS.items():
        fn(ctx, res["helpers"])
    for block in (64, 128, 256, 1024):
        v = 10.0 ** np.linspace(0.0, -300.0, block)
        x = ctx.selftest_helpers("block_suffix_excl", [v], block=block)[0][0]
        true = mr.exact_suffix_excl(v, block)
        rel = mr.errors(x[:-1], true[:-1]) / np.array([float(t) for t in true[:-1]])
        res["helpers"]["block_suffix_excl, %d threads, terms 1 .. 1e-300" % block] = dict(
            points=block, max_rel=float(rel.max()), bar_rel_max=64 * block * mr.EPS, worst_err_over_bar=float(rel.max() / (64 * block * mr.EPS)),
            bar_from="64 nthreads eps: the relative accuracy mwrt_tl_dev.hip.h promises for tiny terms")
    rng = np.random.default_rng(7)
    for block in (64, 128, 256, 1024):                      # bit identity with the order emulations (the tests' property)
        m = 3 * block - 17
        v = rng.standard_normal(m) * np.exp(rng.uniform(-30, 30, m))
        vp = mr.pad(v, block)
        run = lambda name: ctx.selftest_helpers(name, [v], block=block)[0]
        bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)
        scan, tot = mr.emu_block_scan(vp, block)
        got_scan = run("block_scan")
        res["helpers"]["collectives, %d threads" % block] = dict(
            points=m, bar_from="bit-identical to the order emulation",
            block_sum_mismatches=int((bits(run("block_sum")[0]) != bits(mr.emu_block_sum(vp, block)[:m])).sum()),
            block_scan_mismatches=int((bits(got_scan[0]) != bits(scan[:m])).sum() + (bits(got_scan[1]) != bits(tot[:m])).sum()),
            block_suffix_excl_mismatches=int((bits(run("block_suffix_excl")[0]) != bits(mr.emu_block_suffix_excl(vp, block)[:m])).sum()),
            row16_max_mismatches=int((bits(ctx.selftest_helpers("row16_max", [np.abs(vp)], block=block)[0][0])
                                      != bits(mr.emu_row16_max(np.abs(vp)))).sum()))
    n, d = mr.inputs("div_small")
    q = ctx.selftest_helpers("div_small", [n, d])[0][0]
    res["helpers"]["div_small"] = dict(points=int(len(n)), mismatches=int((q != n.astype(np.int64) // d.astype(np.int64)).sum()), bar_from="exact: n // d")
    res["worst_err_over_bar"] = max(r.get("worst_err_over_bar", 0.0) for r in res["helpers"].values())
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
