"""The sorted segment loops of k_tb_fused at the shapes where they can go wrong (GPU, against the C oracle at 1e-6 K).

A sorted K2 pass runs every segment for the full `seglen` layers on a wave-uniform counter, four layers per trip plus a
remainder; the last segment of a row runs past the top level into the row's zero-filled padding.  The level
counts below put that tail at both parities, leave no idle lane to spare, sit on the wave seams and at the top of the
256-thread class, and straddle the level count at which a pass first gets sorted; the frequency counts give one-pass
(5, 8) and two-pass (14 = 8 + 6, 16 = 8 + 8) geometries, the elevation counts different segment splits.
"""
import functools

import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
from oracle import c_oracle

TOL_K = 1e-6
WAVE, NFK, K2_SORT_MIN_SEGLEN = 64, 8, 16
MIN_NLEV = 20                                   # synthetic_profiles needs that many

ELEVATIONS = {1: np.array([90.0]), 3: np.array([90.0, 19.2, 4.2]), 7: pr.BENCH_ELEVATIONS_7}
H = pr.HATPRO_FRQS
FREQUENCIES = {14: H, 8: H[3:11].copy(), 5: H[[0, 6, 7, 10, 13]].copy(), 16: np.sort(np.concatenate([H, [50.3, 60.0]]))}
FIXED_NLEV = (180, 181, 182, 64, 65, 191, 192, 255, 256)


def pick_nfc(nf):
    return (8 if nf <= 8 else 14) if (nf % 14 == 0 or nf <= 14) else 16


def plan_k2_pass(nlev, npairs, threads):
    """csrc/mwrt_plan.cpp plan_k2_pass: segments per (frequency, angle) pair of one K2 pass"""
    layers = nlev - 1
    best, best_cost = 1, -1
    for ns in range(1, min(64, max(layers, 1)) + 1):
        sl = -(-layers // ns)
        rounds = -(-npairs * ns // threads)
        cost = rounds * (sl * 8 + 4) + ns
        if best_cost < 0 or cost < best_cost:
            best, best_cost = ns, cost
    return best


def plan(nlev, nf, nang):
    """(nseg, seglen, sorted) of the K2 passes of the first chunk, and the row stride, as plan_k2 / k_tb_fused have them
    (TB-only clear-sky launch: one lane per level in whole waves; the LDS of these shapes never needs the split shrunk)"""
    threads = -(-nlev // WAVE) * WAVE
    nfc = min(pick_nfc(nf), nf)
    passes = []
    for rows in (min(NFK, nfc), max(0, nfc - NFK)):
        if rows == 0:
            continue
        nseg = plan_k2_pass(nlev, rows * nang, threads)
        seglen = max(1, -(-(nlev - 1) // nseg))
        passes.append((nseg, seglen, rows * nang * nseg <= threads and seglen >= K2_SORT_MIN_SEGLEN))
    ld = max([nlev + 1] + [ns * sl + 1 for ns, sl, _ in passes if sl >= K2_SORT_MIN_SEGLEN])
    return passes, ld + (ld % 2 == 0)


def takes_sorted_path(nlev, nf, nang):
    return any(s for _, _, s in plan(nlev, nf, nang)[0])


@functools.lru_cache(maxsize=None)
def smallest_sorted_nlev(nf, nang):
    """... of the 256-thread class; None where so few pairs are cut into so many segments that none reaches 16 layers"""
    return next((n for n in range(MIN_NLEV, 257) if takes_sorted_path(n, nf, nang)), None)


def level_counts(nf, nang):
    lo = smallest_sorted_nlev(nf, nang)
    return FIXED_NLEV + tuple(n for n in ((lo, lo - 1) if lo else ()) if n >= MIN_NLEV and n not in FIXED_NLEV)


CASES = [(nlev, nf, nang) for nf in FREQUENCIES for nang in ELEVATIONS for nlev in level_counts(nf, nang)]


def test_the_cases_reach_what_they_are_for():
    """(no GPU) the plan the cases rest on: sorted passes with tails of 0, 1 and 2 layers into the padding, remainders of
    the four-layer trip from 0 to 3, one- and two-pass geometries, and an unsorted neighbour below each threshold"""
    tails, rests, npass = set(), set(), set()
    for nlev, nf, nang in CASES:
        passes, ld = plan(nlev, nf, nang)
        npass.add(len(passes))
        for nseg, seglen, srt in passes:
            if srt:
                assert nseg * seglen < ld
                tails.add(nseg * seglen - (nlev - 1))
                rests.add(seglen % 4)
    assert {0, 1, 2, 5} <= tails and rests == {0, 1, 2, 3} and npass == {1, 2}, (tails, rests, npass)
    # 180 levels: three elevations of the 14 channels run sorted with five layers of padding per row; all seven are dealt
    # out over three and two rounds and keep the per-step vote (the neighbour of the sorted path in these tests)
    assert plan(180, 14, 3) == ([(8, 23, True), (10, 18, True)], 185)
    assert plan(180, 14, 7) == ([(10, 18, False), (9, 20, False)], 181)
    for nf in FREQUENCIES:
        for nang in ELEVATIONS:
            lo = smallest_sorted_nlev(nf, nang)
            assert lo is None or (takes_sorted_path(lo, nf, nang) and (lo == MIN_NLEV or not takes_sorted_path(lo - 1, nf, nang)))
    assert sum(smallest_sorted_nlev(nf, nang) is not None for nf in FREQUENCIES for nang in ELEVATIONS) >= 6


@functools.lru_cache(maxsize=None)
def batch(nlev):
    return pr.synthetic_profiles(4, config_id=31, nlev=nlev)


@functools.lru_cache(maxsize=None)
def reference(nlev, nf):
    """oracle TBs of the four profiles at all seven elevations: the 1- and 3-elevation cases use its rows"""
    P = batch(nlev)
    tb, valid = c_oracle.tb_batch(sp.get_model("R24"), P["z"], P["p"], P["t"], P["rh"], FREQUENCIES[nf], ELEVATIONS[7], nthreads=1)
    assert (np.asarray(valid) == 1).all()
    tb = np.asarray(tb).reshape(4, 7, nf)
    tb.setflags(write=False)
    return tb


@pytest.mark.gpu
@pytest.mark.parametrize("nlev,nf,nang", CASES)
def test_segment_loops_match_the_oracle(gpu_ctx, nlev, nf, nang):
    import torch
    P, frq, ang = batch(nlev), FREQUENCIES[nf], ELEVATIONS[nang]
    rows = [int(np.nonzero(ELEVATIONS[7] == a)[0][0]) for a in ang]
    ref = reference(nlev, nf)[:, rows, :]
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(P[k]).to(dev) for k in ("z", "p", "t", "rh")}
    out = torch.full((4, nang, nf), float("nan"), dtype=torch.float64, device=dev)
    val = torch.zeros(4, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.tb_batch_device("R24", 4, nlev, d["z"].data_ptr(), d["p"].data_ptr(), d["t"].data_ptr(), d["rh"].data_ptr(),
                            frq, ang, out.data_ptr(), val.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tb = out.cpu().numpy()
    assert (val.cpu().numpy() == 1).all()
    err = float(np.abs(tb - ref).max())
    print(f"nlev {nlev} nf {nf} nang {nang}: plan {plan(nlev, nf, nang)}  max |TB - oracle| = {err:.3e} K")
    assert np.isfinite(tb).all() and err <= TOL_K
