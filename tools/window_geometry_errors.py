"""What the windowed fine-grid path loses over the geometry table of tests/window_cases.py, per case and model: the numbers
DESIGN.md 4.3 and the k_absorb_win comment quote.

``reference``: the plan's own truncation (tests/window_reference.py plan_truncation: the oracle's line terms through the
dumped nodes and weights, no device involved) over the levels and models tests/test_window_plan.py samples.
``device``: what tests/test_window_geometry.py measures (through tests/window_device.py, which that test uses too):
windowed and every-line absorption against the oracle, windowed against every-line next to the plan's truncation over
all levels, TB against the oracle and the every-line call.  ``bars``: what the tests hold them to.
The file is merged, not replaced: a run without a GPU (--reference-only) keeps the device section it finds.
Usage: python tools/window_geometry_errors.py [--reference-only] [--out profiles/window_geometry_errors.json]"""
import argparse
import json
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
warnings.simplefilter("ignore")

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
import plan_dump_tool as pdt
import window_cases as wc
import window_reference as wr

SAMPLE_LEVELS = (0, 1, 60, 120, 176, 177, 178, 179)


def plans_of(ask, tmp, model_name, cases):
    path = os.path.join(tmp, model_name + ".desc")
    with open(path, "wb") as fh:
        fh.write(bytes(sp.get_model(model_name).to_c()))
    got = ask([pdt.request("tables", path)] + [pdt.request("windows", *c.frq) for c in cases])
    return {c.name: wr.plan_arrays(d, c.frq) for c, d in zip(cases, got[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_geometry_errors.json"))
    ap.add_argument("--reference-only", action="store_true")
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res["units"] = {"reference": "max |interpolated - direct| of the planned far sets, relative to the total dry / wet absorption (sd: "
                                 "the half-sampled speed-dependent shape, relative to wet)",
                    "device": "absorption relative; tb in K; truncation = reference over ALL levels of the three profiles"}
    res["bars"] = {"reference": 5e-10, "absorption_vs_oracle": 1e-9, "windowed_vs_every_line": "truncation + 2e-10",
                   "tb_vs_oracle_K": 1e-6, "tb_vs_every_line_K": 1e-8}
    with tempfile.TemporaryDirectory() as tmp:
        ask = pdt.asker(pdt.build(tmp, sanitise=a.reference_only))      # sanitised runs stay on the CPU side
        P = pr.synthetic_profiles(3, 5)
        column = {k: np.concatenate([P[k][i][list(SAMPLE_LEVELS)] for i in range(3)]) for k in ("p", "t", "rh")}
        ref = {}
        for mn in wc.CPU_MODELS:
            m = sp.get_model(mn)
            for name, plan in plans_of(ask, tmp, mn, wc.CASES).items():
                ref["%s/%s" % (name, mn)] = wr.plan_truncation(plan, m, column)
        res["reference"] = ref
        res["reference_worst"] = {k: max(v[k] for v in ref.values()) for k in ("dry", "wet", "sd")}
        if not a.reference_only:
            import window_device as wd
            from mwr_fast_forward_operators_and_lbls_amd import _native as nat
            ctx = nat.default_context(0)
            dev = {}
            for mn in sorted({mn for c in wc.CASES for mn in c.gpu_models}):
                cases = [c for c in wc.CASES if c.eligible and mn in c.gpu_models]
                plans = plans_of(ask, tmp, mn, cases)
                for c in cases:
                    r = wd.measure(ctx, c, mn, plans[c.name])
                    dev["%s/%s" % (c.name, mn)] = dict(
                        win_vs_oracle=r["win_vs_oracle"], every_vs_oracle=r["every_vs_oracle"],
                        win_vs_every_dry=max(d["dry"] for d in r["win_vs_every"]), win_vs_every_wet=max(d["wet"] for d in r["win_vs_every"]),
                        truncation_dry=max(t["dry"] for t in r["truncation"]), truncation_wet=max(t["wet"] for t in r["truncation"]),
                        truncation_sd=max(t["sd"] for t in r["truncation"]), tb_vs_oracle_K=r["tb_vs_oracle"], tb_vs_every_K=r["tb_vs_every"])
            res["device"] = dev
            res["device_worst"] = {k: max(v[k] for v in dev.values()) for k in next(iter(dev.values()))}
    txt = json.dumps(res, indent=1)
    print(json.dumps({k: res[k] for k in ("reference_worst", "device_worst") if k in res}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
