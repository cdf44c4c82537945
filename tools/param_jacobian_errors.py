"""Largest column errors of the spectroscopic-parameter Jacobian (mwrt_tb_param_jacobian_batch_device) against its exact
reference (tests/param_reference.py: torch autograd of the oracle on the CPU), over the cases of tests/test_param_jacobian.py:
per case the largest |device - reference| of a column over the profile's (elevation, frequency), divided by the column's
largest |entry|, and the parameter it belongs to.  Needs a GPU.
Usage: python tools/param_jacobian_errors.py [--out profiles/param_jacobian_errors.json]"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from mwr_fast_forward_operators_and_lbls_amd import _native as nat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    import param_reference as prf
    import test_param_jacobian as T
    from test_tl_oracle import CASES, edge_profile
    ctx = nat.Context(0)
    res = {"bar": T.TOL_COL, "metric": "max over (elevation, frequency) of |device - reference| / max |reference| per column", "cases": {}}

    def run(what, m, P, frq, ang, params):
        tb, kb, valid = T.device_kb(ctx, m, P, frq, ang, params)
        worst = T.column_errors(m, P, frq, ang, params, kb, tb)
        (name, line), err = max(worst.items(), key=lambda kv: kv[1])
        res["cases"][what] = {"nprof": int(P["z"].shape[0]), "nlev": int(P["z"].shape[1]), "nf": len(frq), "nang": len(ang),
                              "npar": len(params), "max_error": float(err), "at": f"{name}[{'*' if line < 0 else line}]"}
        print(what, res["cases"][what])

    for case in CASES:
        m, sd_frq = T.tables(case)
        sd_line = int(np.argmin(np.abs(np.asarray(m.h2o["fl"]) + 0.3 - sd_frq))) if case.startswith("fuzz") else None
        z, p, t, rh = edge_profile()
        Q = T.profiles(30, 5)
        P = {k: np.stack([x, Q[k][0]]) for k, x in zip(("z", "p", "t", "rh"), (z, p, t, rh))}
        run(case, m, P, T.frequencies(8, sd_frq), T.ELEV, prf.test_params(m, sd_line))
    m, sd_frq = T.tables("R20SD")
    sd_line = int(np.argmax(np.asarray(m.h2o["w2"]) > 0))
    for nlev, nf in [(2, 1), (64, 7), (65, 8), (180, 15)]:
        P = {k: v[:2] for k, v in T.profiles(nlev, 11 + nlev).items()}
        run(f"R20SD nlev {nlev} nf {nf}", m, P, T.frequencies(nf, sd_frq, rot=1), np.array([90.0, 4.2]), T.short_params(m, sd_line))
    m, _ = T.tables("fuzz2")
    run("fuzz2 1024 levels", m, {k: v[:1] for k, v in T.profiles(1024, 3).items()}, np.array([22.235, 60.3061]),
        np.array([90.0, 4.2]), T.short_params(m))
    m, _ = T.tables("R17")
    ang = np.concatenate([np.linspace(4.2, 90.0, 40), np.linspace(91.0, 175.8, 24)])
    run("R17 64 angles", m, {k: v[:1] for k, v in T.profiles(30, 9).items()}, np.array([183.31]), ang, T.short_params(m))
    res["max_error"] = max(c["max_error"] for c in res["cases"].values())
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print("largest:", res["max_error"])


if __name__ == "__main__":
    main()
