"""TEST INFRASTRUCTURE ONLY -- randomly perturbed line tables with randomly flipped model switches.

The generator of ``tests/test_gpu_parity.py::test_fuzzed_tables_and_switches``, copied (that test keeps its inline
copy), so that the K-matrix tests reach the same code paths: shift modes, mixing modes, the 118-GHz line-1 exception,
both N2 variants, speed dependence on any line, exponents that are zero or not."""
from __future__ import annotations

import dataclasses

import numpy as np

from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp


def fuzzed_tables(seed):
    """-> (tables, sd_lines): a ModelTables record named ``fuzz{seed}`` and the indices of its two speed-dependent H2O lines."""
    rng = np.random.default_rng(100 + seed)
    base = sp.get_model(["R98", "R17", "R20SD", "R24"][seed % 4])

    def jig(a, rel=0.05):
        return np.asarray(a) * (1.0 + rel * rng.uniform(-1, 1, np.shape(a)))

    h2o = {k: jig(v) for k, v in base.h2o.items()}
    o2 = {k: jig(v) for k, v in base.o2.items()}
    n = len(h2o["fl"])
    h2o["fl"], o2["f"] = base.h2o["fl"].copy(), base.o2["f"].copy()        # keep centres: cutoffs stay meaningful
    sdl = rng.integers(0, n, 2)                                           # speed dependence on two random lines
    for k in ("w2", "w2s"):
        h2o[k] = np.zeros(n); h2o[k][sdl] = {"w2": 0.4e-3, "w2s": 1.6e-3}[k] * rng.uniform(0.5, 1.5, 2)
    h2o["xw2"] = rng.uniform(0.3, 1.0, n); h2o["xw2s"] = rng.uniform(0.3, 1.3, n)
    h2o["d2"] = np.zeros(n); h2o["d2"][sdl] = rng.uniform(-2e-5, 2e-5, 2)
    h2o["d2s"] = np.zeros(n); h2o["d2s"][sdl] = rng.uniform(-2e-4, 2e-4, 2)
    h2o["aair"] = rng.uniform(0, 1, n) * (rng.random(n) < 0.3)
    h2o["aself"] = rng.uniform(0, 10, n) * (rng.random(n) < 0.3)
    h2o["xh"] = rng.uniform(0, 2.5, n) * (rng.random(n) < 0.5)
    h2o["xhs"] = rng.uniform(0, 1.0, n) * (rng.random(n) < 0.5)
    h2o["sh"] = rng.uniform(-2e-4, 2e-4, n); h2o["shs"] = rng.uniform(-1.5e-3, 1.5e-3, n)
    mix = int(rng.integers(0, 2))
    if mix:
        m = len(o2["f"])
        o2["g0"] = rng.uniform(-0.3, 0.2, m); o2["g1"] = rng.uniform(-0.6, 0.2, m)
        o2["dnu0"] = rng.uniform(-0.05, 0.05, m); o2["dnu1"] = rng.uniform(-0.03, 0.03, m)
    tab = dataclasses.replace(
        base, name=f"fuzz{seed}", h2o=h2o, o2=o2,
        h2o_shift_mode=int(rng.choice([0, 2])), o2_mix_mode=mix, o2_line1_dens=int(rng.integers(0, 2)),
        n2_fdep=int(rng.integers(0, 2)), n2_ptot=int(rng.integers(0, 2)),
        o2_x=float(rng.uniform(0.7, 0.85)), o2_wv_factor=float(rng.uniform(1.0, 1.3)),
        h2o_reftline=float(rng.choice([296.0, 300.0])), t_cosmic=float(rng.uniform(2.6, 2.8)))
    return tab, sdl
