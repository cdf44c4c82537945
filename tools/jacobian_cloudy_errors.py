"""The largest errors of the cloudy device K-matrix (mwrt_tb_jacobian_batch_opt_device) against the exact derivative
reference, per check: the numbers DESIGN.md 4.5.2 records.  Runs the cases of tests/test_jacobian_cloudy.py (its
helpers) and prints one JSON object.  Needs a GPU.

    python tools/jacobian_cloudy_errors.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_jacobian_cloudy as C  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import _native  # noqa: E402


def main():
    ctx = _native.Context(0)
    try:
        out = {}
        for case in C.CASES:
            for key, v in C.cloudy_case_errors(ctx, *case).items():
                out[key] = max(out.get(key, 0.0), v)
        for nlev, name in C.SLAB_CASES:
            for key, v in C.cloudy_case_errors(ctx, nlev, name, 3, 2, kind="slab", frq=C.SLAB_FRQ).items():
                out[f"slab {key}"] = max(out.get(f"slab {key}", 0.0), v)
        # reported, not asserted anywhere: the isothermal slab at 58 GHz, where the reference itself is ill-conditioned
        for nlev, name in ((12, "R98"), (65, "R24"), (180, "R98")):
            err = C.cloudy_case_errors(ctx, nlev, name, 3, 2, kind="slab", frq=C.FRQ)
            out[f"slab at 58 GHz, {nlev} levels (reference ill-conditioned)"] = {k: err[k] for k in ("dtb_dliq", "dtb_dice")}
        out.update({f"autograd {key}": v for key, v in C.autograd_errors().items()})
    finally:
        ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
