#!/usr/bin/env python3
"""Low elevations along refracted ray paths (needs a GPU).  First the geometry error itself: plane-parallel minus ray-traced
TB of one synthetic sounding at 30, 10.2 and 4.2 degrees, from the device.  Then one retrieval: the observations are made
by the ray-traced forward operator at seven elevations down to 4.2 degrees, and retrieval.OneDVar retrieves them with
Levenberg-Marquardt damping twice -- with ray_tracing=True (mwrt_tb_jacobian_batch_ray_device: the same operator and its
exact K rows) and without (the plane-parallel K-matrix, which carries the geometry error in F(x) and in K).

    python examples/low_elevation_retrieval.py
"""
import os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import _native, profiles as pr, retrieval
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables

warnings.simplefilter("ignore")
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
ctx = _native.default_context(0)

# ---- the geometry error -------------------------------------------------------------------------------------------------
P = pr.synthetic_profiles(3, 73)
frq3, elev3 = np.array([22.24, 31.4, 51.26]), np.array([30.0, 10.2, 4.2])
z, p, t, rh = (dev(P[k][:1]) for k in ("z", "p", "t", "rh"))
tbs = []
for rays in (False, True):
    tb = torch.empty((1, elev3.size, frq3.size), dtype=torch.float64, device="cuda")
    valid = torch.empty(1, dtype=torch.uint8, device="cuda")
    ctx.tb_batch_device("R24", 1, z.shape[1], z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq3, elev3,
                        tb.data_ptr(), valid.data_ptr(), ray_tracing=rays)
    ctx.synchronize()
    tbs.append(tb.cpu().numpy()[0])
print("plane-parallel TB minus ray-traced TB [K] (synthetic profile, R24)")
print("elevation   " + "   ".join(f"{f:6.2f} GHz" for f in frq3))
for a, row in zip(elev3, tbs[0] - tbs[1]):
    print(f"{a:6.1f} deg  " + "   ".join(f"{d:10.2f}" for d in row))

# ---- one retrieval of ray-made observations, with and without rays ------------------------------------------------------------
NPROF, NLEV = 100, pr.N_LEVELS
frq, elev = pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()
zm = P["z"].mean(axis=0)
corr = np.exp(-np.abs(zm[:, None] - zm[None, :]) / 1.5)
sig_t, sig_h = 2.0, 0.08
sa = np.zeros((2 * NLEV, 2 * NLEV))
sa[:NLEV, :NLEV] = sig_t ** 2 * corr
sa[NLEV:, NLEV:] = sig_h ** 2 * corr
rng = np.random.default_rng(11)
draw = rng.standard_normal((NPROF, 2 * NLEV)) @ np.linalg.cholesky(sa + 1e-10 * np.eye(2 * NLEV)).T
xa = x_true + dev(draw.reshape(NPROF, 2, NLEV))
xa[:, 1].clamp_(min=0.0)
xa = xa.contiguous()
noise = 0.3
se = dev(np.full(frq.size * elev.size, noise ** 2))


def one_d_var(rays):
    return retrieval.OneDVar("R24", frq, elev, dev(sa), se, variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=xa,
                             ray_tracing=rays)


tb_true = one_d_var(True).forward(z, p, x_true)[0]
y = tb_true + noise * torch.randn(tb_true.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
below = torch.tensor(zm < 4.0, device="cuda")
m = frq.size * elev.size
print(f"\n{NPROF} soundings, y = ray-traced F(x_true) + {noise} K noise at {frq.size} channels x {elev.size} elevations "
      f"({elev.min():.1f} ... {elev.max():.1f} deg), retrieve_lm")
for rays in (True, False):
    res = one_d_var(rays).retrieve_lm(z, p, y, max_iter=20, tol=0.05)
    ok = res.converged
    rms = lambda blk: float(((res.x[:, blk][:, below] - x_true[:, blk][:, below]) ** 2).mean(dim=1).sqrt()[ok].median())   # noqa: E731
    print(f"ray_tracing={str(rays):5s}  converged {int(ok.sum()):3d} of {NPROF}   chi2/m median {float((res.chi2[ok] / m).median()):7.2f}"
          f"   RMS below 4 km  T {rms(0):.3f} K  rh {rms(1):.4f}")
