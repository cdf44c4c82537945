#!/usr/bin/env python3
"""The device K-matrix in the variables a retrieval works in (needs a GPU): RTTOV-gb's K run for a batch of soundings in
one device call per elevation -- dTB/dT at fixed ppmv, dTB/dppmv and dTB/dliq [K per kg/kg] per level and channel, with
the hydrostatic heights folded in inside the kernel -- printed as the text block the reference's parser walks
(python_src/proc/RTTOV_gb_processing.py:286-300).

    python examples/k_matrix_in_retrieval_variables.py
"""
import os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, rttov_gb_wrapper as rw

warnings.simplefilter("ignore")
NPROF = 40
P = pr.synthetic_profiles(NPROF, 7)
profs = []
for i in range(NPROF):
    z, p, t, rh = (P[k][i] for k in ("z", "p", "t", "rh"))
    e = rh * rw.goff_gratch_es(t)
    liquid = np.where((z > 1.0) & (z < 1.6), 3e-4, 0.0)        # a 600-m liquid cloud, 0.3 g/kg
    profs.append({"p": p[::-1].copy(), "t": t[::-1].copy(), "ppmv": (e / p * 1e6)[::-1].copy(), "liquid": liquid[::-1].copy(),
                  "t2m": t[0], "ps": p[0], "height_km": z[0], "lat": 50.0, "zenith": 0.0 if i % 2 else 60.0})
rw.jacobians_batch(profs, "R24", liquid=True)                 # warm-up (tables, workspace, first launches)
t0 = time.perf_counter()
d_t, d_q, d_l = rw.jacobians_batch(profs, "R24", liquid=True)
t1 = time.perf_counter()
print(f"K-matrix of {NPROF} soundings, 180 levels x 14 channels, two elevations: {1e3 * (t1 - t0):.1f} ms "
      f"(arrays {d_t.shape}, host transfers included)")
print("58-GHz temperature weights of sounding 1 sum to", round(float(d_t[1][:, 13].sum()), 4))
text = rw.format_jacobians(profs[1]["p"], d_t[1], d_q[1], d_l[1])
print("".join(text.splitlines(keepends=True)[:3 + 6]), "  ...")
jac = rw.parse_jacobians(text, 180)
print("parsed back:", jac.shape, " largest |dTB/dliq| of channel 7 (31.4 GHz):", f"{np.abs(jac[:, 6, 3]).max():.4g} K per kg/kg")
