#!/usr/bin/env python3
"""The 1D-Var of examples/one_d_var_retrieval.py in a reduced basis (needs a GPU).  A ground-based radiometer
resolves a handful of degrees of freedom per profile, so instead of 2 x 180 level values the retrieval estimates r = 24
coefficients of the leading eigenvectors (EOFs) of the prior covariance's blocks, x = xa + B c: mwrt_basis_project_device contracts
the K rows with B behind the K-matrix call, and the optimal-estimation entries run on the one block K B [m][r].  The same
synthetic observations are retrieved in the full state and in the basis (Levenberg-Marquardt both), and the example prints
degrees of freedom, errors below 4 km, trial counts and wall time side by side -- the basis once with the representation
error of the truncated eigenvectors in Se and once without, which shows why it belongs there.  A second part adds a liquid
cloud whose profile shape is known and retrieves one more coefficient: the factor that scales it (a liquid-water-path
retrieval).

    python examples/reduced_basis_retrieval.py
"""
import os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis

warnings.simplefilter("ignore")
NPROF, NLEV, R = 200, pr.N_LEVELS, 24
frq, elev = pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()          # state blocks: T [K], rh [fraction]

# the prior of examples/one_d_var_retrieval.py: every sounding's own first guess, off the truth by a draw from Sa
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
m = frq.size * elev.size
se = dev(np.full(m, noise ** 2))
variables = JacVariables.of(humidity="rh")

# EOFs per block, 12 of temperature and 12 of humidity, side by side as one block-diagonal B [360][24]: the eigenvectors of
# the whole Sa would all be temperature, whose variance in K^2 dwarfs that of a humidity in fractions
eof_t, eof_h = (StateBasis.from_covariance(torch.tensor(sa[i * NLEV:(i + 1) * NLEV, i * NLEV:(i + 1) * NLEV]), R // 2) for i in (0, 1))
eof = StateBasis(torch.block_diag(eof_t.b, eof_h.b), torch.block_diag(eof_t.sa_c, eof_h.sa_c))       # c_a = 0: the prior is xa
kept = float(torch.diagonal(eof_t.sa_c).sum()) / np.trace(sa[:NLEV, :NLEV])
print(f"{R // 2} of {NLEV} eigenvectors per block carry {100 * kept:.1f} % of the block's prior variance")
full = retrieval.OneDVar("R24", frq, elev, dev(sa), se, variables=variables, blocks=("t", "h"), xa=xa)
# What the basis cannot represent still reaches the radiometer.  Seen through K, the truncated part of the prior,
# Sa - B sa_c B^T, is observation error of the reduced retrieval (representation error); with the noise alone in Se the 24
# coefficients absorb signal that is not theirs.  K is the batch mean at the first guess, Se a full [m][m] shared by the batch.
k_blocks, _ = full._linearise(z, p, xa)
k_mean = torch.cat([k.reshape(NPROF, m, NLEV) for k in k_blocks], dim=2).mean(dim=0)
b_dev, lam_dev = eof.b.to("cuda"), eof.sa_c.to("cuda")
rep = k_mean @ (dev(sa) - b_dev @ lam_dev @ b_dev.T) @ k_mean.T
se_red = (torch.diag(se) + 0.5 * (rep + rep.T)).contiguous()
red = retrieval.OneDVar("R24", frq, elev, None, se_red, variables=variables, blocks=("t", "h"), xa=xa, basis=eof)
bare = retrieval.OneDVar("R24", frq, elev, None, se, variables=variables, blocks=("t", "h"), xa=xa, basis=eof)
tb_true = full.forward(z, p, x_true)[0]
y = tb_true + noise * torch.randn(tb_true.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
below = torch.tensor(zm < 4.0, device="cuda")                                  # where a ground-based radiometer sees


def err(a, blk, truth=x_true):
    """RMS of a - truth below 4 km, per profile."""
    return ((a[:, blk][:, below] - truth[:, blk][:, below]) ** 2).mean(dim=1).sqrt()


def timed(ov):
    ov.retrieve_lm(z, p, y, max_iter=1)                                        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ov.retrieve_lm(z, p, y, max_iter=20, tol=0.05)
    torch.cuda.synchronize()
    return res, 1e3 * (time.perf_counter() - t0)


runs = [("full state (n = 360)", *timed(full)), ("basis (r = %d)" % R, *timed(red)), ("basis, noise-only Se", *timed(bare))]
print(f"\n{NPROF} profiles x {NLEV} levels x {m} observations, Levenberg-Marquardt, tol 0.05 sigma")
print(f"{'':40s}" + "".join(f"{name:>24s}" for name, _, _ in runs))
rows = [("converged", lambda r, ms: f"{int(r.converged.sum())} of {NPROF}"),
        ("trials, median / most", lambda r, ms: f"{int(r.iterations.median())} / {int(r.iterations.max())}"),
        ("wall time [ms]", lambda r, ms: f"{ms:.1f}"),
        ("dfs, median", lambda r, ms: f"{float(r.dfs.median()):.2f}"),
        ("chi2 / m, median", lambda r, ms: f"{float((r.chi2 / m).median()):.2f}"),
        ("T error below 4 km [K], median", lambda r, ms: f"{float(err(r.x, 0).median()):.3f}"),
        ("rh error below 4 km, median", lambda r, ms: f"{float(err(r.x, 1).median()):.4f}"),
        ("posterior sigma of T at the ground [K]", lambda r, ms: f"{float(r.post_var[:, 0, 0].sqrt().median()):.2f}")]
for name, cell in rows:
    print(f"{name:40s}" + "".join(f"{cell(r, ms):>24s}" for _, r, ms in runs))
print(f"(first guess: T {float(err(xa, 0).median()):.3f} K, rh {float(err(xa, 1).median()):.4f}; the posterior sigma of a basis run "
      f"leaves out the prior variance outside its span)")

# ---- a liquid cloud of known shape: one more column, the factor that scales it ----
shape = np.where((zm > 1.0) & (zm < 1.6), 0.2, 0.0)                            # g m-3: the cloud of scale 1
lwp = float((0.5 * (shape[1:] + shape[:-1]) * np.diff(zm)).sum())              # kg m-2 (g m-3 x km)
scale_true = dev(rng.uniform(0.2, 2.5, NPROF))
x_true3 = torch.cat([x_true, (scale_true[:, None] * dev(shape)[None, :])[:, None, :]], dim=1).contiguous()
xa3 = torch.cat([xa, torch.zeros_like(xa[:, :1])], dim=1).contiguous()         # the liquid block is B c alone
b3 = np.zeros((3 * NLEV, R + 1))
b3[:2 * NLEV, :R] = eof.b.numpy()
b3[2 * NLEV:, R] = shape
sa_c3 = np.diag(np.concatenate([np.diag(eof.sa_c.numpy()), [1.0]]))            # the scale factor: prior 1 +- 1
c_a3 = np.concatenate([np.zeros(R), [1.0]])
cloudy = retrieval.OneDVar("R24", frq, elev, None, se_red, variables=variables, blocks=("t", "h", "liq"), xa=xa3,
                           basis=StateBasis(torch.tensor(b3), torch.tensor(sa_c3), c_a=torch.tensor(c_a3)))
tb3 = cloudy.forward(z, p, x_true3)[0]
y = tb3 + noise * torch.randn(tb3.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
res_c, ms_c = timed(cloudy)
ok = res_c.converged
got = res_c.coeff[:, R]
print(f"\nwith a liquid cloud of known shape ({1e3 * lwp:.0f} g m-2 at scale 1) and r = {R} + 1: {int(ok.sum())} of {NPROF} converged, "
      f"{ms_c:.1f} ms")
print(f"liquid water path: RMS error {1e3 * lwp * float(((got - scale_true)[ok] ** 2).mean().sqrt()):.1f} g m-2 over truths of "
      f"{1e3 * lwp * float(scale_true.min()):.0f} .. {1e3 * lwp * float(scale_true.max()):.0f} g m-2 (prior: {1e3 * lwp:.0f} +- {1e3 * lwp:.0f})")
print(f"T error below 4 km [K], median: {float(err(res_c.x, 0, x_true3)[ok].median()):.3f};  dfs, median: {float(res_c.dfs[ok].median()):.2f}")
