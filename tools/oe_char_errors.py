"""Largest error of every output of mwrt_oe_gain_device and of the chain gain -> mwrt_oe_product_device against the NumPy
reference (tests/oe_char_reference.py), over the shapes and variants tests/test_oe_char.py runs, in the units of that
test's bars (oe_char_reference.char_errors); the bar itself is 1e-8.  Also the product entry alone on the reference's own
gain, in units of its element-wise bound 2 m eps |gain|^T |K| (resp. 2 m eps (|Sa| + |gain|^T |W|)); that bar is 1.
Usage: python tools/oe_char_errors.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import oe_char_reference as ocr
import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native as nat

dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")   # noqa: E731
cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731


def gain(ctx, case):
    k = [dev(b) for b in case["k"]]
    nprof, m, nlev = k[0].shape
    nblk, n = len(k), len(k) * nlev
    x, xa, sa, se, y, fx = (dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(gain=torch.empty((nprof, m, n), **f64), ksa=torch.empty((nprof, m, n), **f64),
               keep=torch.empty((nprof, m), dtype=torch.uint8, device="cuda"), avk_diag=torch.empty_like(x),
               dfs_block=torch.empty((nprof, nblk), **f64), noise_var=torch.empty_like(x), smooth_var=torch.empty_like(x),
               status=torch.empty(nprof, dtype=torch.uint8, device="cuda"))
    ctx.oe_gain_device(nprof, nlev, m, [b.data_ptr() for b in k], x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(),
                       y.data_ptr(), fx.data_ptr(), out["status"].data_ptr(), d_gain=out["gain"].data_ptr(),
                       d_ksa=out["ksa"].data_ptr(), d_keep=out["keep"].data_ptr(), d_avk_diag=out["avk_diag"].data_ptr(),
                       d_dfs_block=out["dfs_block"].data_ptr(), d_noise_var=out["noise_var"].data_ptr(),
                       d_smooth_var=out["smooth_var"].data_ptr(), xa_per_profile=case["xa"].ndim == 3,
                       se_full=case["se"].ndim == 2, stream=cur())
    return k, sa, out


def product(ctx, which, g, keep, k, ksa, sa, rows):
    nprof, m, n = g.shape
    r0, rc = rows or (0, 0)
    out = torch.empty((nprof, rc or n, n), dtype=torch.float64, device="cuda")
    ctx.oe_product_device(nprof, n // len(k), m, which, g.data_ptr(), keep.data_ptr(), out.data_ptr(), [b.data_ptr() for b in k],
                          d_ksa=ksa.data_ptr(), d_sa=sa.data_ptr(), row_begin=r0, row_count=rc, stream=cur())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.Context(0)
    keys = ("gain", "ksa", "avk_diag", "dfs_block", "noise_var", "smooth_var", "avk", "post_cov")
    res = {"bar": oer.TOL, "cases": {}, "max": {k: 0.0 for k in keys}, "max_cond": 0.0,
           "product_alone_in_units_of_its_bound": {"avk": 0.0, "post_cov": 0.0}}
    for nlev, nblk, m in oer.SHAPES:
        n = nblk * nlev
        windows = [None] if n < 2048 else [(0, n // 2), (n // 2, n // 2)]
        for se_full in (False, True):
            for xa_pp in (False, True):
                case = oer.make_case(nlev, nblk, m, nprof=4, se_full=se_full, xa_per_profile=xa_pp)
                k, sa, out = gain(ctx, case)
                torch.cuda.synchronize()
                got = {key: v.cpu().numpy() for key, v in out.items()}
                err = {}
                for rows in windows:
                    ref = ocr.oe_char_reference(**case, rows=rows)
                    got["avk"] = product(ctx, nat.OE_PRODUCT_AVK, out["gain"], out["keep"], k, out["ksa"], sa, rows)
                    got["post_cov"] = product(ctx, nat.OE_PRODUCT_POST_COV, out["gain"], out["keep"], k, out["ksa"], sa, rows)
                    for key, v in ocr.char_errors(got, ref, case, rows=rows).items():
                        err[key] = max(err.get(key, 0.0), v)
                    if not se_full and not xa_pp:                  # the product alone, on exact inputs
                        r0, rc = rows or (0, n)
                        g, kp, w = dev(ref["gain"]), dev(ref["keep"]), dev(ref["ksa"])
                        K = np.concatenate(case["k"], axis=2)
                        a_ref, a_b = ocr.product_reference(ref["gain"], ref["keep"], K, rows=rows)
                        s_ref, s_b = ocr.product_reference(ref["gain"], ref["keep"], ref["ksa"], sa=case["sa"], rows=rows)
                        ea = np.abs(product(ctx, nat.OE_PRODUCT_AVK, g, kp, k, w, sa, rows) - a_ref) / (2 * m * ocr.EPS * a_b)
                        es = np.abs(product(ctx, nat.OE_PRODUCT_POST_COV, g, kp, k, w, sa, rows) - s_ref) / \
                            (2 * m * ocr.EPS * (np.abs(case["sa"][r0:r0 + rc])[None] + s_b))
                        pa = res["product_alone_in_units_of_its_bound"]
                        pa["avk"], pa["post_cov"] = max(pa["avk"], float(ea.max())), max(pa["post_cov"], float(es.max()))
                err["cond"] = float(np.nanmax(ref["cond"]))
                res["cases"][f"{nlev}-{nblk}-{m}-{'full' if se_full else 'diag'}-{'perprofile' if xa_pp else 'shared'}"] = err
                for key in res["max"]:
                    res["max"][key] = max(res["max"][key], err[key])
                res["max_cond"] = max(res["max_cond"], err["cond"])
    txt = json.dumps(res, indent=1)
    print(json.dumps({"max": res["max"], "max_cond": res["max_cond"], "product_alone": res["product_alone_in_units_of_its_bound"]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
