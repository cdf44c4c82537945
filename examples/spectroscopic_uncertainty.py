#!/usr/bin/env python3
"""How far the brightness temperatures move when the spectroscopy moves (needs a GPU): the spectroscopic-parameter
Jacobian K_b of the 14 HATPRO channels (sensitivity.param_jacobian), the 1-sigma TB uncertainty
sqrt(diag K_b S_b K_b^T) it implies at zenith and at 4.2 degrees, the five parameters that dominate each channel, and the
1D-Var example with and without that forward-model term in Se (Rodgers 2000, section 3.2.2).

THE RELATIVE UNCERTAINTIES BELOW ARE ILLUSTRATIVE PLACEHOLDERS, NOT PUBLISHED VALUES: round numbers of a plausible
size, uncorrelated.  The published uncertainty budgets (e.g. Cimini et al. 2018) could not be restated offline, and this
project does not restate numbers it cannot check.  Replace SIGMA_REL (and add covariances) with real values.

    python examples/spectroscopic_uncertainty.py
"""
import os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval, sensitivity
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables

warnings.simplefilter("ignore")
MODEL = "R24"
# ILLUSTRATIVE PLACEHOLDERS (see above): 1-sigma RELATIVE uncertainty of each parameter
SIGMA_REL = {
    "h2o_cf": 0.05, "h2o_cs": 0.10, "h2o_xcf": 0.05, "h2o_xcs": 0.05, "o2_x": 0.05, "o2_wb300": 0.10, "n2_l": 0.05,
    "h2o_s1[0]": 0.01, "h2o_w0[0]": 0.02, "h2o_w0s[0]": 0.03, "h2o_x[0]": 0.05, "h2o_sh[0]": 0.10,
    "o2_s300[*]": 0.01, "o2_w300[*]": 0.02, "o2_y0[*]": 0.05, "o2_y1[*]": 0.10, "o2_g0[*]": 0.10, "o2_dnu0[*]": 0.10,
}
NPROF, NLEV = 100, pr.N_LEVELS
frq, elev = pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
z, p, t, rh = (dev(P[k]) for k in ("z", "p", "t", "rh"))

recs = sensitivity.parse_params(MODEL, list(SIGMA_REL))
tb, kb, valid = sensitivity.param_jacobian(MODEL, z, p, t, rh, frq, elev, recs, relative=True)   # K per unit relative change
sb = torch.tensor([s ** 2 for s in SIGMA_REL.values()], dtype=torch.float64, device="cuda")
cov = sensitivity.model_error_covariance(kb, sb)                       # [nprof][m][m], m = nang * nf
sig = cov.diagonal(dim1=1, dim2=2).sqrt().reshape(NPROF, elev.size, frq.size).mean(dim=0).cpu().numpy()
part = (kb ** 2 * sb).mean(dim=0).cpu().numpy()                        # [nang][nf][npar]: each parameter's variance share

print(f"{MODEL}, {NPROF} synthetic soundings; relative uncertainties: ILLUSTRATIVE PLACEHOLDERS")
print("channel [GHz]   1-sigma TB [K] at 90 deg / 4.2 deg    the five parameters that dominate (zenith), share of the variance")
a_zen, a_low = int(np.argmin(np.abs(elev - 90.0))), int(np.argmin(np.abs(elev - 4.2)))
for j, f in enumerate(frq):
    share = part[a_zen, j] / part[a_zen, j].sum()
    top = np.argsort(share)[::-1][:5]
    print(f"{f:8.2f}        {sig[a_zen, j]:6.3f} / {sig[a_low, j]:6.3f}       " + ", ".join(f"{recs[q].label} {100 * share[q]:.0f}%" for q in top))

# the 1D-Var of examples/one_d_var_retrieval.py with Se = noise alone and with Se = noise + mean K_b S_b K_b^T; the
# observations are simulated with a PERTURBED spectroscopy (one draw from S_b, through K_b), which the retrieval does not know
zm = P["z"].mean(axis=0)
corr = np.exp(-np.abs(zm[:, None] - zm[None, :]) / 1.5)
sa = np.zeros((2 * NLEV, 2 * NLEV))
sa[:NLEV, :NLEV] = 2.0 ** 2 * corr
sa[NLEV:, NLEV:] = 0.08 ** 2 * corr
rng = np.random.default_rng(11)
x_true = torch.stack([t, rh], dim=1).contiguous()
xa = x_true + dev((rng.standard_normal((NPROF, 2 * NLEV)) @ np.linalg.cholesky(sa + 1e-10 * np.eye(2 * NLEV)).T).reshape(NPROF, 2, NLEV))
xa[:, 1].clamp_(min=0.0)
xa = xa.contiguous()
noise = 0.3
m_obs = frq.size * elev.size
db = dev(rng.standard_normal(len(recs))) * sb.sqrt()                    # one relative perturbation of the spectroscopy
gen = torch.Generator("cuda").manual_seed(1)
y = tb + (kb @ db) + noise * torch.randn(tb.shape, dtype=torch.float64, device="cuda", generator=gen)
se_noise = torch.full((m_obs,), noise ** 2, dtype=torch.float64, device="cuda")
se_model = torch.diag(se_noise) + sensitivity.model_error_covariance(kb, sb, reduce="mean")
below = torch.tensor(zm < 4.0, device="cuda")
for label, se in (("Se = noise alone", se_noise), ("Se = noise + K_b S_b K_b^T", se_model)):
    ov = retrieval.OneDVar(MODEL, frq, elev, dev(sa), se, variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=xa)
    res = ov.retrieve_lm(z, p, y, max_iter=20, tol=0.05)
    ok = res.converged
    rms = lambda blk: float(((res.x[:, blk][:, below] - x_true[:, blk][:, below]) ** 2).mean(dim=1).sqrt()[ok].median())   # noqa: E731
    print(f"{label:28s} converged {int(ok.sum())} of {NPROF};  RMS below 4 km  T {rms(0):.3f} K  rh {rms(1):.4f};  "
          f"chi2 / m median {float((res.chi2[ok] / m_obs).median()):.2f}")
