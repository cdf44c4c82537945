"""The largest errors of the device K-matrix path against the exact derivative reference, per check: the numbers
DESIGN.md 4.5.1 records.  Runs the same cases as tests/test_jacobian_device_edges.py (its helpers) and prints one JSON
object.  Needs a GPU.

    python tools/jacobian_edge_errors.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_jacobian_device_edges as E  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import _native  # noqa: E402


def main():
    ctx = _native.Context(0)
    try:
        out = {"absorption value": 0.0, "absorption tangent": 0.0, "absorption entries at a branch threshold": 0}
        for name in E.ABS_MODELS:
            err = E.absorption_errors(ctx, name)
            out["absorption value"] = max(out["absorption value"], err["value"])
            out["absorption tangent"] = max(out["absorption tangent"], err["tangent"])
            out["absorption entries at a branch threshold"] += err["branch"]
        k = {key: 0.0 for key in ("TB", "dtb_dt", "dtb_de", "dtb_ddz")}
        for case in E.KCASES:
            for key, v in E.k_case_errors(ctx, *case).items():
                k[key] = max(k[key], v)
        for key, v in E.thin_64_angle_errors(ctx).items():
            k[key] = max(k[key], v)
        out.update({f"K-matrix {key}": v for key, v in k.items()})
        out.update({f"autograd {key}": v for key, v in E.autograd_errors().items()})
    finally:
        ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
