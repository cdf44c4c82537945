#!/usr/bin/env python3
"""What a 1D-Var retrieval from a ground-based radiometer resolves (needs a GPU): a few synthetic soundings are retrieved
with the set-up of one_d_var_retrieval.py (14 HATPRO channels x 7 elevations, state = T and rh on the model levels), and
OneDVar.characterise returns the averaging kernel, the gain and the error budget of the result (mwrt_oe_gain_device and
mwrt_oe_product_device).  Printed: the degrees of freedom for signal per state block, which add up to the
retrieval's dfs; for three levels the height at which the temperature averaging-kernel row peaks and its width; and the
split of the posterior temperature error into smoothing and measurement noise there.

    python examples/averaging_kernels.py
"""
import os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables

warnings.simplefilter("ignore")
NPROF, NLEV = 8, pr.N_LEVELS
frq, elev = pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()          # state blocks: T [K], rh [fraction]

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
noise = 0.3                                                                    # K
se = np.full(frq.size * elev.size, noise ** 2)

ov = retrieval.OneDVar("R24", frq, elev, dev(sa), dev(se), variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=xa)
tb_true = ov.forward(z, p, x_true)[0]
y = tb_true + noise * torch.randn(tb_true.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(1))

res = ov.retrieve_lm(z, p, y, max_iter=20, tol=0.05)                           # its diagnostics are those of the state returned
ch = ov.characterise(z, p, res.x, y, avk=True, rows=(0, NLEV))                 # the temperature rows of A are enough here
torch.cuda.synchronize()

ok = res.converged & (ch.status == 1)
print(f"{NPROF} profiles x {NLEV} levels x {se.size} observations; converged: {int(ok.sum())} of {NPROF}")
print("degrees of freedom for signal      T      rh     sum    retrieval's dfs")
for i in range(NPROF):
    d = ch.dfs_block[i]
    print(f"  profile {i}                     {float(d[0]):5.2f}  {float(d[1]):5.2f}  {float(d.sum()):6.3f}  {float(res.dfs[i]):6.3f}")
worst = float((ch.dfs_block.sum(dim=1) - res.dfs).abs().max())
print(f"largest |sum over blocks - dfs|: {worst:.1e}")

# rows of the temperature averaging kernel, per unit height: A[j, k] / dz_k against z_k
a_tt = ch.avk[:, :, :NLEV].mean(dim=0).cpu().numpy()                           # [level j][level k], mean over the soundings
dz = np.gradient(zm)
print("\nT averaging-kernel rows (mean over the soundings)")
print("  level at      row peaks at   width (area / peak)   A_jj    sigma: prior -> smoothing, noise, total")
for target in (0.5, 2.0, 5.0):
    j = int(np.argmin(np.abs(zm - zm[0] - target)))
    row = a_tt[j] / dz                                                         # [1 / km]
    k = int(np.argmax(row))
    width = float(a_tt[j].sum() / row[k]) if row[k] > 0 else float("nan")
    sm = float(ch.smooth_var[:, 0, j].mean().clamp(min=0).sqrt())
    nz = float(ch.noise_var[:, 0, j].mean().sqrt())
    print(f"  {zm[j] - zm[0]:5.2f} km      {zm[k] - zm[0]:5.2f} km        {width:5.2f} km            {a_tt[j, j]:5.3f}   "
          f"{sig_t:.1f} K -> {sm:.2f} K, {nz:.2f} K, {np.hypot(sm, nz):.2f} K")
