#!/usr/bin/env python3
"""What the antenna beam and the channel bandpass do to a HATPRO-like radiometer (needs a GPU): instrument.Instrument turns
the monochromatic pencil-beam forward operator into a channel model.

  1  channel minus monochromatic TB per channel at 90 / 30 / 10.2 / 5.4 / 4.2 deg, for a 3.5 deg Gaussian beam and boxcar bands
  2  the convergence of the quadrature: 2, 3, 5 band nodes and 3, 5 beam nodes (where 5 nodes stay above the horizon)
     against the finest rule.  The band rule of a channel that holds a narrow line core of the humid upper levels
     (22.24 GHz on the synthetic profile) does NOT converge with a few Gauss-Legendre nodes: give such a channel an explicit
     (offsets, weights) pair that resolves the line
  3  a Levenberg-Marquardt retrieval of observations synthesised WITH the instrument, once retrieved with it and once with
     the monochromatic pencil-beam operator

    python examples/instrument_response.py
"""
import os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument

warnings.simplefilter("ignore")
frq = pr.HATPRO_FRQS
elev = np.array([90.0, 30.0, 10.2, 5.4, 4.2])
bands = [0.23] * 10 + [0.6, 0.6, 1.0, 2.0]                                      # GHz, widening towards 58 GHz
FWHM = 3.5
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
variables = JacVariables.of(humidity="rh")


def channel_tb(inst, z, p, t, rh):
    """TBs of an instrument for profiles on the device: one K-matrix call on its grid, one reduction."""
    stream = torch.cuda.current_stream().cuda_stream
    tb, _, _ = retrieval._native_k_matrix("R98", z, p, t, rh, None, None, inst.frq_q, inst.elev_q, variables, ("t", "h"), stream)
    return inst.apply(tb)[0].cpu().numpy()


def table(title, rows, d):
    print(title)
    print("  elev  " + " ".join(f"{f:7.2f}" for f in frq))
    for el, r in zip(rows, d):
        print(f"  {el:5.1f} " + " ".join(f"{v:+7.3f}" for v in r))


P = pr.synthetic_profiles(2, nlev=60)
z, p, t, rh = (dev(P[k][:1]) for k in ("z", "p", "t", "rh"))
centre = channel_tb(Instrument(frq, elev), z, p, t, rh)[0]
full = channel_tb(Instrument(frq, elev, beam=FWHM, band=bands, n_beam=3, n_band=3), z, p, t, rh)[0]
beam = channel_tb(Instrument(frq, elev, beam=FWHM, n_beam=3), z, p, t, rh)[0]
band = channel_tb(Instrument(frq, elev, band=bands, n_band=3), z, p, t, rh)[0]
table(f"\n1  channel minus monochromatic pencil-beam TB [K] ({FWHM} deg beam, 3 nodes; boxcar bands, 3 nodes)", elev, full - centre)
table("   the beam alone", elev, beam - centre)
table("   the band alone", elev, band - centre)

print("\n2  convergence of the quadrature [K]")
fine = channel_tb(Instrument(frq, elev, band=bands, n_band=9), z, p, t, rh)[0]
for n in (2, 3, 5):
    d = channel_tb(Instrument(frq, elev, band=bands, n_band=n), z, p, t, rh)[0] - fine
    print(f"   {n} band nodes minus 9: largest |difference| per channel  " + " ".join(f"{v:7.3f}" for v in np.abs(d).max(axis=0)))
print("   (a channel whose difference does not fall with n holds a line core narrower than its node spacing -- 22.24 GHz here;\n"
      "    no claim is made for it: hand that channel an explicit (offsets, weights) pair)")
high = elev[elev > 4.3]                                                         # 5 nodes of a 3.5 deg beam reach 4.25 deg down
b3 = channel_tb(Instrument(frq, high, beam=FWHM, n_beam=3), z, p, t, rh)[0]
b5 = channel_tb(Instrument(frq, high, beam=FWHM, n_beam=5), z, p, t, rh)[0]
table("   5 beam nodes minus 3 (4.2 deg left out: the outermost of 5 nodes would look below the horizon)", high, b5 - b3)
try:
    Instrument(frq, elev, beam=FWHM, n_beam=5)
except ValueError as err:
    print("   ", err)

print("\n3  retrieve_lm on observations made WITH the instrument")
NPROF, NLEV = 100, pr.N_LEVELS
r_elev = pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()
zm = P["z"].mean(axis=0)
corr = np.exp(-np.abs(zm[:, None] - zm[None, :]) / 1.5)
sig_t, sig_h, noise = 2.0, 0.08, 0.5
sa = np.zeros((2 * NLEV, 2 * NLEV))
sa[:NLEV, :NLEV] = sig_t ** 2 * corr
sa[NLEV:, NLEV:] = sig_h ** 2 * corr
rng = np.random.default_rng(11)
draw = rng.standard_normal((NPROF, 2 * NLEV)) @ np.linalg.cholesky(sa + 1e-10 * np.eye(2 * NLEV)).T
xa = x_true + dev(draw.reshape(NPROF, 2, NLEV))
xa[:, 1].clamp_(min=0.0)
xa = xa.contiguous()
m = frq.size * r_elev.size
se = dev(np.full(m, noise ** 2))
inst = Instrument(frq, r_elev, beam=FWHM, band=bands, n_beam=3, n_band=3)
with_inst = retrieval.OneDVar("R24", frq, r_elev, dev(sa), se, variables=variables, blocks=("t", "h"), xa=xa, instrument=inst)
without = retrieval.OneDVar("R24", frq, r_elev, dev(sa), se, variables=variables, blocks=("t", "h"), xa=xa)
tb_true = with_inst.forward(z, p, x_true)[0]
y = tb_true + noise * torch.randn(tb_true.shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
below = torch.tensor(zm < 4.0, device="cuda")


def err_below(a, blk):
    return ((a[:, blk][:, below] - x_true[:, blk][:, below]) ** 2).mean(dim=1).sqrt()


print(f"   {NPROF} profiles, {m} channels x elevations, sigma(Se) = {noise} K; prior error below 4 km, median: "
      f"T {float(err_below(xa, 0).median()):.3f} K, rh {float(err_below(xa, 1).median()):.4f}")
for name, ov in (("with the instrument   ", with_inst), ("monochromatic, pencil ", without)):
    res = ov.retrieve_lm(z, p, y, max_iter=20, tol=0.05)
    ok = res.converged
    print(f"   {name}: converged {int(ok.sum())} of {NPROF}, chi2 / m median {float((res.chi2 / m).median()):.2f}, "
          f"error below 4 km, median: T {float(err_below(res.x, 0).median()):.3f} K, rh {float(err_below(res.x, 1).median()):.4f}")
