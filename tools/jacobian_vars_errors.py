"""The largest errors of the device K-matrix in retrieval variables against the chained exact reference, per row kind:
the numbers DESIGN.md 4.5.3 records.  Runs the cases of tests/test_kmatrix_variables.py (its helpers: all 12 mode
combinations per case) and the wrapper check, and prints one JSON object.  Needs a GPU.

    python tools/jacobian_vars_errors.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_kmatrix_variables as V  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import _native  # noqa: E402


def main():
    ctx = _native.Context(0)
    try:
        worst = {key: 0.0 for key in ("TB",) + V.KEYS}
        per_case = {}
        for case in V.CASES:
            err = V.case_errors(ctx, *case)
            per_case["-".join(str(c) for c in case)] = err
            for key, v in err.items():
                worst[key] = max(worst[key], v)
        out = {"of the row's largest sum of absolute terms (TB: relative)": worst, "per case": per_case,
               "jacobians_batch vs end-to-end autograd": V.wrapper_errors()[0]}
    finally:
        ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
