#!/usr/bin/env python3
"""Which observations of a scan carry the information (needs a GPU).  The 14 channels x 16 elevations of
examples/many_observation_retrieval.py are 224 candidate observations per profile; that example can only compare the whole
16-elevation scan with the fixed 7-elevation one.  selection.rank_observations ranks all 224 at the first guess, with the
12 + 12 EOF basis of that example: every round mwrt_oe_select_device takes the observation that reduces the entropy of the
current posterior most, assimilates it and goes on.  Printed: the degrees of freedom for signal after 14, 49, 98 and 224
picks against the dfs of the fixed 7-elevation scan (98 observations), which elevations and which frequencies fill the first
98 picks, and how early the picks stop paying.

    python examples/scan_strategy.py
"""
import os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval, selection
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis

warnings.simplefilter("ignore")
NPROF, NLEV, R = 200, pr.N_LEVELS, 24
frq = pr.HATPRO_FRQS
elev16 = np.round(90.0 * np.sin(np.linspace(np.arcsin(5.4 / 90.0), np.pi / 2, 16)), 1)[::-1].copy()   # 90 .. 5.4 degrees
elev7 = pr.BENCH_ELEVATIONS_7
P = pr.synthetic_profiles(NPROF, 7)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
z, p = dev(P["z"]), dev(P["p"])
x_true = torch.stack([dev(P["t"]), dev(P["rh"])], dim=1).contiguous()

# the prior and the basis of examples/many_observation_retrieval.py
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


def make(elev):
    eof = StateBasis(torch.block_diag(eof_t.b, eof_h.b), torch.block_diag(eof_t.sa_c, eof_h.sa_c))
    m = frq.size * elev.size
    return retrieval.OneDVar("R24", frq, elev, None, dev(np.full(m, noise ** 2)), variables=variables, blocks=("t", "h"), xa=xa,
                             basis=eof, form="n")


c0 = torch.zeros((NPROF, R), dtype=torch.float64, device="cuda")           # the first guess: the prior
ov16, ov7 = make(elev16), make(elev7)
m16, m7 = ov16.m, ov7.m
sel = selection.rank_observations(ov16, z, p, c0)
fixed = selection.rank_observations(ov7, z, p, c0)                          # all 98 of the fixed scan: its dfs, whatever the order
torch.cuda.synchronize()
assert sel.status.cpu().tolist() == [1] * NPROF and fixed.status.cpu().tolist() == [1] * NPROF
print(f"{NPROF} profiles x {NLEV} levels, r = {R}; {m16} candidates = {frq.size} channels x {elev16.size} elevations {elev16.tolist()}")
dfs7 = float(fixed.cum_dfs[:, -1].median())
print(f"the fixed scan, {m7} observations at {elev7.tolist()}: dfs {dfs7:.2f}, {float(fixed.cum_info[:, -1].median()):.1f} bits")
for k in (14, 49, 98, 224):
    print(f"the best {k:3d} of {m16}: dfs {float(sel.cum_dfs[:, k - 1].median()):.2f} ({float(sel.cum_dfs[:, k - 1].median()) / dfs7:.2f} of the "
          f"fixed scan's), {float(sel.cum_info[:, k - 1].median()):.1f} bits")
reach = (sel.cum_dfs >= fixed.cum_dfs[:, -1:]).float().argmax(dim=1) + 1
print(f"picks needed to reach the fixed scan's dfs: median {int(reach.median())}, at most {int(reach.max())}")

# which elevations and which frequencies fill the first 98: observation = elevation * nf + frequency
first = sel.first(98).reshape(elev16.size, frq.size).cpu().numpy()          # in how many profiles each is among them
print("share of the first 98 picks by elevation (degrees: picks per profile of the 14 possible):")
print("  " + ", ".join(f"{e:g}: {n / NPROF:.1f}" for e, n in zip(elev16, first.sum(axis=1))))
print("share of the first 98 picks by frequency (GHz: picks per profile of the 16 possible):")
print("  " + ", ".join(f"{f:g}: {n / NPROF:.1f}" for f, n in zip(frq, first.sum(axis=0))))
head = sel.order[:, :14].cpu().numpy()
common = np.bincount(head.reshape(-1), minlength=m16).argsort()[::-1][:14]
print("the 14 observations most often among a profile's first 14 (elevation, GHz): "
      + ", ".join(f"({elev16[j // frq.size]:g}, {frq[j % frq.size]:g})" for j in common))
left = sel.q_left.clone()
print(f"after all {m16}: nothing is left to add (largest remaining q {float(left[sel.rank < 0].max()) if bool((sel.rank < 0).any()) else 0.0:.1e}); "
      f"the last pick added {float(sel.info_bits[:, -1].median()):.1e} bits against {float(sel.info_bits[:, 0].median()):.2f} of the first")
