#!/usr/bin/env python3
"""A 1D-Var with more observations than the m-form takes (needs a GPU).  14 channels x 16 elevations are 224
observations per profile; the m-form of the optimal-estimation step holds an m x m matrix in LDS and stops at 140.  The
n-form, OneDVar(form="n"), solves an n x n system for the r = 12 + 12 EOF coefficients of examples/reduced_basis_retrieval.py
instead -- mwrt_oe_nform_prepare_device streams K B once, mwrt_oe_nform_solve_device factorises a 24 x 24 matrix -- and has
no limit on m.  The example retrieves the 16-elevation scan with form="n" (Levenberg-Marquardt), shows that form="m" is
refused there, at 14 x 7 = 98 observations prints both forms side by side, and ends with what the extra elevations buy:
OneDVar.characterise_nform gives the degrees of freedom per block and the temperature averaging kernels at 7
and at 16 elevations.  The n-form takes variances only, so what the 24 coefficients cannot represent enters Se as the diagonal
of its representation error K (Sa - B sa_c B^T) K^T, with K the batch mean at the first guess
(examples/reduced_basis_retrieval.py carries the full matrix, which the m-form can take).

    python examples/many_observation_retrieval.py
"""
import os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables, MwrtError
from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis

warnings.simplefilter("ignore")
NPROF, NLEV, R = 200, pr.N_LEVELS, 24
frq = pr.HATPRO_FRQS
elev16 = np.round(90.0 * np.sin(np.linspace(np.arcsin(5.4 / 90.0), np.pi / 2, 16)), 1)[::-1].copy()   # 90 .. 5.4 degrees
P = pr.synthetic_profiles(NPROF, 7)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()

# the prior and the basis of examples/reduced_basis_retrieval.py: 12 EOFs of temperature and 12 of humidity
zm = P["z"].mean(axis=0)
corr = np.exp(-np.abs(zm[:, None] - zm[None, :]) / 1.5)
sa = np.zeros((2 * NLEV, 2 * NLEV))
sa[:NLEV, :NLEV] = 2.0 ** 2 * corr
sa[NLEV:, NLEV:] = 0.08 ** 2 * corr
rng = np.random.default_rng(11)
draw = rng.standard_normal((NPROF, 2 * NLEV)) @ np.linalg.cholesky(sa + 1e-10 * np.eye(2 * NLEV)).T
xa = x_true + dev(draw.reshape(NPROF, 2, NLEV))
xa[:, 1].clamp_(min=0.0)
xa = xa.contiguous()
eof_t, eof_h = (StateBasis.from_covariance(torch.tensor(sa[i * NLEV:(i + 1) * NLEV, i * NLEV:(i + 1) * NLEV]), R // 2) for i in (0, 1))
variables = JacVariables.of(humidity="rh")
noise = 0.3
below = torch.tensor(zm < 4.0, device="cuda")


def make(elev, form):
    eof = StateBasis(torch.block_diag(eof_t.b, eof_h.b), torch.block_diag(eof_t.sa_c, eof_h.sa_c))
    m = frq.size * elev.size
    ov = retrieval.OneDVar("R24", frq, elev, None, dev(np.full(m, noise ** 2)), variables=variables, blocks=("t", "h"), xa=xa,
                           basis=eof, form=form)
    k_blocks = ov._observe(z, p, xa, project=False)[2]                         # the unprojected rows at the first guess
    k_mean = torch.cat([k.reshape(NPROF, m, NLEV) for k in k_blocks], dim=2).mean(dim=0)
    b, lam = eof.b.to("cuda"), eof.sa_c.to("cuda")
    rep = torch.einsum("ij,jk,ik->i", k_mean, dev(sa) - b @ lam @ b.T, k_mean)
    se = (noise ** 2 + rep.clamp(min=0.0)).contiguous()
    return retrieval.OneDVar("R24", frq, elev, None, se, variables=variables, blocks=("t", "h"), xa=xa, basis=eof, form=form)


def observe(ov, seed):
    tb = ov.forward(z, p, x_true)[0]
    return tb + noise * torch.randn(tb.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


def timed(ov, y):
    ov.retrieve_lm(z, p, y, max_iter=1)                                        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ov.retrieve_lm(z, p, y, max_iter=20, tol=0.05)
    torch.cuda.synchronize()
    return res, 1e3 * (time.perf_counter() - t0)


def report(name, res, ms, m):
    err = lambda blk: float(((res.x[:, blk][:, below] - x_true[:, blk][:, below]) ** 2).mean(dim=1).sqrt().median())   # noqa: E731
    print(f"{name:28s} converged {int(res.converged.sum()):3d} of {NPROF}, trials {int(res.iterations.median())} / {int(res.iterations.max())}, "
          f"{ms:7.1f} ms, dfs {float(res.dfs.median()):.2f}, chi2/m {float((res.chi2 / m).median()):.2f}, "
          f"T {err(0):.3f} K, rh {err(1):.4f} below 4 km")


# ---- 14 x 16 = 224 observations: the n-form alone ----
m16 = frq.size * elev16.size
ov16 = make(elev16, "n")
y16 = observe(ov16, 1)
print(f"{NPROF} profiles x {NLEV} levels, r = {R}; elevations {elev16.tolist()}")
res16, ms16 = timed(ov16, y16)
report(f"form='n', m = {m16}", res16, ms16, m16)
try:
    make(elev16, "m").step(z, p, res16.coeff, y16)
except MwrtError as e:
    print(f"form='m', m = {m16}: refused -- {e}")

# ---- 14 x 7 = 98 observations: both forms side by side ----
elev7 = pr.BENCH_ELEVATIONS_7
m7 = frq.size * elev7.size
ov_m, ov_n = make(elev7, "m"), make(elev7, "n")
y7 = observe(ov_m, 2)
res_m, ms_m = timed(ov_m, y7)
res_n, ms_n = timed(ov_n, y7)
report(f"form='m', m = {m7}", res_m, ms_m, m7)
report(f"form='n', m = {m7}", res_n, ms_n, m7)
print(f"largest difference of the two forms: coefficients {float((res_n.coeff - res_m.coeff).abs().max() / res_m.coeff.abs().max()):.1e} "
      f"of the largest, post_var {float((res_n.post_var - res_m.post_var).abs().max() / res_m.post_var.max()):.1e}")
print(f"16 elevations against 7: T error below 4 km {float(((res16.x[:, 0][:, below] - x_true[:, 0][:, below]) ** 2).mean(dim=1).sqrt().median()):.3f} K "
      f"against {float(((res_n.x[:, 0][:, below] - x_true[:, 0][:, below]) ** 2).mean(dim=1).sqrt().median()):.3f} K, "
      f"dfs {float(res16.dfs.median()):.2f} against {float(res_n.dfs.median()):.2f}")

# ---- what the extra elevations buy: the characterisation of the n-form step ----
# characterise_nform works in the 24 coefficients: the first 12 are temperature EOFs, the last 12 humidity EOFs, so the
# degrees of freedom per physical block are the two halves of the averaging-kernel diagonal.  The EOFs are orthonormal, so a
# temperature row of the level-space averaging kernel is (B_t A_tt B_t^T)[level, :].
half = R // 2
ch16 = ov16.characterise_nform(z, p, res16.coeff, y16, gain=False, avk=True)
ch7 = ov_n.characterise_nform(z, p, res_n.coeff, y7, gain=False, avk=True)
for name, ch in (("7 elevations ", ch7), ("16 elevations", ch16)):
    d = ch.avk_diag[:, 0]
    print(f"{name}: dfs T {float(d[:, :half].sum(dim=1).median()):.2f}, rh {float(d[:, half:].sum(dim=1).median()):.2f}; "
          f"noise share of the posterior variance of the leading T coefficient "
          f"{float((ch.noise_var[:, 0, 0] / (ch.noise_var[:, 0, 0] + ch.smooth_var[:, 0, 0])).median()):.2f}")
b_t = eof_t.b.to("cuda")
for name, ch in (("7 elevations ", ch7), ("16 elevations", ch16)):
    rows = (b_t @ ch.avk[:, :half, :half].mean(dim=0) @ b_t.T).cpu().numpy()          # the batch-mean T kernel in level space
    for target in (0.5, 1.5, 4.0):
        k = int(np.argmin(np.abs(zm - target)))
        w = rows[k]
        above = np.flatnonzero(w >= 0.5 * w.max())
        print(f"{name}: T averaging kernel of the level at {zm[k]:.2f} km peaks at {zm[int(np.argmax(w))]:.2f} km, "
              f"half-width {zm[above.max()] - zm[above.min()]:.2f} km, area {w.sum():.2f}")
