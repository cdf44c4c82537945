#!/usr/bin/env python3
"""An observation-error covariance of its own for every profile (needs a GPU).  The reduced-basis retrieval of
examples/reduced_basis_retrieval.py leaves the truncated part of the prior to Se as representation error, K S_res K^T, and
that matrix depends on each scene's own K: a humid scene seen at low elevation and a dry one at zenith do not share it.
The example retrieves the same synthetic observations three ways -- the representation error per profile through ``se=``
(mwrt_obs_whiten_device pre-whitens every linearisation, the update entries run with Se = 1), its batch mean as the one
shared Se, and the noise alone -- and prints chi2 / m and the errors below 4 km side by side.  A fourth run adds a
per-profile spectroscopic error K_b S_b K_b^T (sensitivity.model_error_covariance) whose parameter uncertainties are the
ILLUSTRATIVE PLACEHOLDERS of examples/spectroscopic_uncertainty.py, not a spectroscopic assessment.

    python examples/scene_dependent_error.py
"""
import os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval, sensitivity
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis

warnings.simplefilter("ignore")
NPROF, NLEV, R = 200, pr.N_LEVELS, 24
frq, elev = pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()

# the prior, the noise and the basis of examples/reduced_basis_retrieval.py
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
noise = 0.3                                                                    # K
m = frq.size * elev.size
se_noise = dev(np.full(m, noise ** 2))
variables = JacVariables.of(humidity="rh")
eof_t, eof_h = (StateBasis.from_covariance(torch.tensor(sa[i * NLEV:(i + 1) * NLEV, i * NLEV:(i + 1) * NLEV]), R // 2) for i in (0, 1))
eof = StateBasis(torch.block_diag(eof_t.b, eof_h.b), torch.block_diag(eof_t.sa_c, eof_h.sa_c))
eof.sa_res = torch.block_diag(eof_t.sa_res, eof_h.sa_res)                       # what the 24 columns leave out of Sa
ov = retrieval.OneDVar("R24", frq, elev, None, se_noise, variables=variables, blocks=("t", "h"), xa=xa, basis=eof)
tb_true = ov.forward(z, p, x_true)[0]
y = tb_true + noise * torch.randn(tb_true.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(1))

# the representation error of every profile at its first guess, and its batch mean
rep = ov.representation_error(z, p, xa)                                        # [nprof][m][m]
se_p = (torch.diag(se_noise)[None] + rep).contiguous()
se_mean = se_p.mean(dim=0).contiguous()
sd = rep.diagonal(dim1=1, dim2=2).sqrt()
print(f"representation error of r = {R}, 1-sigma per observation [K]: median {float(sd.median()):.2f}, "
      f"over the batch {float(sd.min()):.2f} .. {float(sd.max()):.2f}; largest ratio between two profiles on one channel "
      f"{float((sd.amax(dim=0) / sd.amin(dim=0)).max()):.1f}")
mean_ov = retrieval.OneDVar("R24", frq, elev, None, se_mean, variables=variables, blocks=("t", "h"), xa=xa, basis=eof)
below = torch.tensor(zm < 4.0, device="cuda")


def err(a, blk):
    return ((a[:, blk][:, below] - x_true[:, blk][:, below]) ** 2).mean(dim=1).sqrt()


def timed(o, **kw):
    o.retrieve_lm(z, p, y, max_iter=1, **kw)                                   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = o.retrieve_lm(z, p, y, max_iter=20, tol=0.05, **kw)
    torch.cuda.synchronize()
    return res, 1e3 * (time.perf_counter() - t0)


runs = [("per profile (se=)", *timed(ov, se=se_p)), ("batch mean", *timed(mean_ov)), ("noise only", *timed(ov))]

# a per-profile spectroscopic error on top: K_b S_b K_b^T with PLACEHOLDER uncertainties
SIGMA_REL = {"h2o_cf": 0.05, "h2o_cs": 0.10, "o2_x": 0.05, "h2o_w0[0]": 0.02, "o2_w300[*]": 0.02, "o2_y0[*]": 0.05}
recs = sensitivity.parse_params("R24", list(SIGMA_REL))
_, kb, _ = sensitivity.param_jacobian("R24", z, p, xa[:, 0].contiguous(), xa[:, 1].contiguous(), frq, elev, recs, relative=True)
sb = torch.tensor([s ** 2 for s in SIGMA_REL.values()], dtype=torch.float64, device="cuda")
se_spec = (se_p + sensitivity.model_error_covariance(kb, sb)).contiguous()
runs.append(("+ K_b S_b K_b^T (placeholders)", *timed(ov, se=se_spec)))

print(f"\n{NPROF} profiles x {NLEV} levels x {m} observations, r = {R}, Levenberg-Marquardt, tol 0.05 sigma; Se = noise + ...")
print(f"{'':40s}" + "".join(f"{name:>32s}" for name, _, _ in runs))
rows = [("converged", lambda r, ms: f"{int(r.converged.sum())} of {NPROF}"),
        ("trials, median / most", lambda r, ms: f"{int(r.iterations.median())} / {int(r.iterations.max())}"),
        ("wall time [ms]", lambda r, ms: f"{ms:.1f}"),
        ("dfs, median", lambda r, ms: f"{float(r.dfs.median()):.2f}"),
        ("chi2 / m, median", lambda r, ms: f"{float((r.chi2 / m).median()):.2f}"),
        ("chi2 / m, 10 % .. 90 %", lambda r, ms: f"{float((r.chi2 / m).quantile(0.1)):.2f} .. {float((r.chi2 / m).quantile(0.9)):.2f}"),
        ("T error below 4 km [K], median", lambda r, ms: f"{float(err(r.x, 0).median()):.3f}"),
        ("T error below 4 km [K], worst tenth", lambda r, ms: f"{float(err(r.x, 0).quantile(0.9)):.3f}"),
        ("rh error below 4 km, median", lambda r, ms: f"{float(err(r.x, 1).median()):.4f}")]
for name, cell in rows:
    print(f"{name:40s}" + "".join(f"{cell(r, ms):>32s}" for _, r, ms in runs))
print(f"(first guess: T {float(err(xa, 0).median()):.3f} K, rh {float(err(xa, 1).median()):.4f}; the observations carry noise alone, "
      "so the last column shows what a larger Se costs, not what it buys)")
