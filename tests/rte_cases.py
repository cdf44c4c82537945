"""Hand-built columns for the two K2 kernels, each made to reach one thing, with the CPU restatement of the route it takes.

entry "tau":   k_rte_tau<NA> through mwrt_tb_from_layer_tau_device -- tau [nprof][nlev][nf] (zenith, per layer), T, valid.
entry "alpha": the K2 passes of k_tb_fused<ALPHA> through mwrt_tb_from_absorption_device -- awet, adry [nprof][nf][nlev], z, T.
               Most alpha cases use a constant coefficient per (profile, frequency) (the layer rule's |d| < 1e-9 branch returns
               it exactly) and choose the layer THICKNESS: tau[i][j] = a[j] dz[i], so a layer of zero thickness is an exact no-op.

`tau_votes` restates the votes of k_rte_tau (csrc/mwrt_tau.hip.h), `alpha_plan` / `alpha_routes` the plan and the loops of
k_tb_fused's K2 passes as launch_fused starts the from-absorption variant (csrc/mwrt.hip, mwrt_plan.cpp, mwrt_fused.hip.h).
tests/test_rte_reference.py asserts, per case, the route it is built for, and that every case but the dedicated threshold
ones (THRESHOLD_CASES) keeps tau * airmass at least MARGIN away from the switches, so that the restated route is the device's.
"""
import functools

import numpy as np

import math_reference as mr
import rte_reference as rr

WAVE, NFK, K2_SORT_MIN_SEGLEN, GRP = 64, 8, 16, 16
MARGIN = 1e-9
FLOAT_MARGIN = 1e-6                 # ... of the float maxima of a sorted pass (one float ulp is 6e-8)
TINY, THIN = mr.EXP_TINY_X, mr.EXP_SMALL_X
E3 = np.array([90.0, 19.2, 4.2])
E7 = np.array([90.0, 42.0, 30.0, 19.2, 10.2, 5.4, 4.2])


class Case:
    def __init__(self, name, entry, t, frq, elev, tau=None, awet=None, adry=None, z=None, valid=None, pitch_extra=0, held=True):
        self.name, self.entry, self.held, self.pitch_extra = name, entry, held, pitch_extra
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.frq, self.elev = np.asarray(frq, dtype=np.float64), np.asarray(elev, dtype=np.float64)
        self.nprof, self.nlev = self.t.shape
        self.nf, self.nang = len(self.frq), len(self.elev)
        self.am = rr.airmass(self.elev)
        if entry == "tau":
            self.tau = np.ascontiguousarray(tau, dtype=np.float64)
            assert self.tau.shape == (self.nprof, self.nlev, self.nf), (name, self.tau.shape)
            self.valid = np.ones(self.nprof, dtype=np.uint8) if valid is None else np.asarray(valid, dtype=np.uint8)
        else:
            self.awet, self.adry = np.ascontiguousarray(awet, dtype=np.float64), np.ascontiguousarray(adry, dtype=np.float64)
            self.z = np.ascontiguousarray(z, dtype=np.float64)
            assert self.awet.shape == self.adry.shape == (self.nprof, self.nf, self.nlev) and self.z.shape == self.t.shape, name

    @functools.cached_property
    def layer(self):
        """alpha: (tau in longdouble, its relative bar, the flags the kernel must write)"""
        return rr.layer_tau(self.awet, self.adry, self.z)

    @property
    def tau_ld(self):
        return self.tau if self.entry == "tau" else self.layer[0]

    @property
    def valid_expected(self):
        return self.valid if self.entry == "tau" else self.layer[2]

    def nan_expected(self):
        """outputs that are NaN by contract: a flagged profile, a NaN elevation's rows, a frequency whose column holds a NaN"""
        m = np.zeros((self.nprof, self.nang, self.nf), dtype=bool)
        m[self.valid_expected != 1] = True
        m[:, np.isnan(self.elev), :] = True
        if self.entry == "tau":
            m |= np.isnan(self.tau[:, 1:, :]).any(axis=1)[:, None, :]
        return m

    @functools.cached_property
    def reference(self):
        c = rr.model_consts()
        if self.entry == "tau":
            return rr.evaluate(self.tau, self.t, self.frq, self.am, c)
        tau, rel, _ = self.layer
        nseg = max(ns for ns, _, _ in alpha_plan(self.nlev, self.nf, self.nang)["passes"])
        return rr.evaluate(tau, self.t, self.frq, self.am, c, dtau_rel=rel, planck_lanes="level", nseg=nseg)


def rng_of(name):
    return np.random.default_rng([20250301, sum(map(ord, name))])


def temps(nprof, nlev, lo=215.0, hi=292.0, rng=None):
    t = np.tile(np.linspace(hi, lo, nlev), (nprof, 1))
    return t if rng is None else t + rng.uniform(-2.0, 2.0, t.shape)


def loguniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


HATPRO = np.array([22.24, 23.04, 23.84, 25.44, 26.24, 27.84, 31.4, 51.26, 52.28, 53.86, 54.94, 56.66, 57.3, 58.0])


# ---------------------------------------------------------------------------------------------------------------------
# the restated routes
# ---------------------------------------------------------------------------------------------------------------------
def rte_tau_angles(rem):
    return rem if rem <= 8 else (10 if rem == 10 else (5 if rem == 9 else 8))


def angle_groups(nang):
    out, a0 = [], 0
    while a0 < nang:
        na = rte_tau_angles(nang - a0)
        out.append((a0, na))
        a0 += na
    return out


def tau_votes(case):
    """k_rte_tau's votes, in the device's own double arithmetic: per launch group g a dict with
    step [nprof][nwave][nlev-1] (0 tiny, 1 thin, 2 general: the wave's vote at the group's longest path),
    elev_thin [nprof][nwave][nlev-1][na] (inside the general branch: that elevation's step voted thin), and over all groups
    `margin`: the smallest relative distance of a compared product from its switch."""
    tau = case.tau[:, 1:, :]
    nw = -(-case.nf // WAVE)
    groups, margin = [], np.inf
    for a0, na in angle_groups(case.nang):
        am = case.am[a0:a0 + na]
        am_max = 0.0
        for v in am:
            am_max = np.fmax(am_max, abs(v))                       # fmax: a NaN air mass is passed over
        with np.errstate(invalid="ignore", over="ignore"):
            prod = np.abs(tau) * am_max
            tl = np.abs(tau[..., None] * am)                        # [P][L-1][F][na]
        step = np.zeros((case.nprof, nw, case.nlev - 1), dtype=int)
        ethin = np.zeros((case.nprof, nw, case.nlev - 1, na), dtype=bool)
        for w in range(nw):
            s = slice(w * WAVE, min(case.nf, (w + 1) * WAVE))       # idle lanes repeat the last frequency: no new value
            not_tiny = (prod[:, :, s] > TINY).any(axis=2)
            not_thin = (prod[:, :, s] > THIN).any(axis=2)
            step[:, w, :] = not_tiny.astype(int) + not_thin.astype(int)
            ethin[:, w] = ~(tl[:, :, s, :] > THIN).any(axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            for thr in (TINY, THIN):
                d = np.abs(prod / thr - 1)
                margin = min(margin, np.nanmin(np.where(np.isfinite(d), d, np.inf)))
            d = np.abs(tl / THIN - 1)
            margin = min(margin, np.nanmin(np.where(np.isfinite(d), d, np.inf)))
        groups.append(dict(a0=a0, na=na, am_max=am_max, step=step, elev_thin=ethin))
    return groups, float(margin)


def plan_k2_pass(nlev, npairs, threads):
    """csrc/mwrt_plan.cpp plan_k2_pass"""
    layers = nlev - 1
    best, best_cost = 1, -1
    for ns in range(1, min(64, max(layers, 1)) + 1):
        sl = -(-layers // ns)
        cost = -(-npairs * ns // threads) * (sl * 8 + 4) + ns
        if best_cost < 0 or cost < best_cost:
            best, best_cost = ns, cost
    return best


def pick_nfc(nf):
    return (8 if nf <= 8 else 14) if (nf % 14 == 0 or nf <= 14) else 16


def alpha_plan(nlev, nf, nang):
    """the launch of the from-absorption variant: launch_fused gives it 256 threads where one lane per level in whole waves
    would be fewer and there is more than one elevation (a fourth wave that holds no level but takes work items); the chunk
    width, the segment split of the two passes, the row stride and the loop each pass runs.  (The shapes of this table are far
    from the LDS limit that would shrink the split.)"""
    threads = -(-nlev // WAVE) * WAVE
    if threads < 256 and nang > 1:
        threads = 256
    nfc = pick_nfc(nf)
    rows = (min(NFK, nfc, nf), max(0, min(nfc, nf) - NFK))
    passes = []
    for r in rows:
        nseg = plan_k2_pass(nlev, r * nang, threads) if r else 1
        passes.append((nseg, max(1, -(-(nlev - 1) // nseg)), r))
    ld = max([nlev + 1] + [ns * sl + 1 for ns, sl, _ in passes if sl >= K2_SORT_MIN_SEGLEN])
    ld += ld % 2 == 0
    kinds = []
    for ns, sl, r in passes:
        if r == 0:
            continue
        srt = r * nang * ns <= threads and sl >= K2_SORT_MIN_SEGLEN
        kinds.append("sorted" if srt else ("vote" if ns * sl < ld else "short"))
    return dict(threads=threads, nfc=nfc, passes=[p for p in passes if p[2]], ld=ld, kinds=kinds)


def alpha_routes(case):
    """per chunk and pass of an alpha case: the loop kind, and for a sorted pass the loops its waves take per profile
    ({"thin", "general", "mixed"}), the float maxima's margin and `unsafe`: the largest tau * airmass / (1/8) of any layer
    that an item dealt to the thin loop holds; for a vote pass the number of steps voted thin and general."""
    plan = alpha_plan(case.nlev, case.nf, case.nang)
    tz = np.asarray(case.tau_ld, dtype=np.float64)                  # [P][L][F]; row 0 is no layer
    L, nang, threads = case.nlev, case.nang, plan["threads"]
    out = []
    for c0 in range(0, case.nf, plan["nfc"]):
        nfc = min(plan["nfc"], case.nf - c0)
        for h, ((nseg, seglen, _), kind) in enumerate(zip(plan["passes"], plan["kinds"])):
            nfk = min(NFK, nfc - h * NFK)
            if nfk <= 0:
                continue
            items = nfk * nang * nseg
            it = np.arange(items)
            pr, seg = it // nseg, it % nseg
            jj, a = pr // nang, pr % nang
            lo = 1 + seg * seglen
            rec = dict(chunk=c0, h=h, kind=kind, nseg=nseg, seglen=seglen, items=items)
            pad = np.zeros((case.nprof, max(plan["ld"], nseg * seglen + 1) + 8, nfk))
            pad[:, :L, :] = np.where(case.valid_expected[:, None, None] == 1, tz[:, :, c0 + h * NFK:c0 + h * NFK + nfk], 0.0)
            pad[:, 0, :] = 0.0
            layers = lo[:, None] + np.arange(seglen)[None, :]                       # [items][seglen]
            tl = np.abs(pad[:, layers, jj[:, None]] * case.am[a][None, :, None])    # [P][items][seglen]
            real = (layers < L)[None]
            if kind == "sorted":
                ngrp = threads // GRP
                f32 = np.zeros((case.nprof, ngrp * GRP, nfk), dtype=np.float32)
                with np.errstate(over="ignore"):
                    f32[:, :L, :] = pad[:, :L, :].astype(np.float32) * np.float32(1.0000005)
                gmax = f32.reshape(case.nprof, ngrp, GRP, nfk).max(axis=2)            # [P][ngrp][nfk]
                hi = np.minimum(lo + seglen, L)
                gm = np.zeros((case.nprof, items), dtype=np.float32)
                for k in range(items):
                    g0, g1 = lo[k] // GRP, (hi[k] - 1) // GRP
                    if g1 >= g0:
                        gm[:, k] = gmax[:, g0:g1 + 1, jj[k]].max(axis=1)
                with np.errstate(invalid="ignore"):
                    prod = gm.astype(np.float64) * case.am[a][None, :]
                    thin = ~(prod > THIN)
                    rec["float_margin"] = float(np.nanmin(np.abs(prod / THIN - 1)))
                rec["nthin"] = thin.sum(axis=1)
                loops = []
                for p in range(case.nprof):
                    kinds = set()
                    for w0 in range(0, items, WAVE):
                        w1 = min(items, w0 + WAVE)
                        kinds.add("thin" if w1 <= rec["nthin"][p] else ("general" if w0 >= rec["nthin"][p] else "mixed"))
                    loops.append(kinds)
                rec["loops"] = loops
                worst = np.where(thin[:, :, None] & real, tl, 0.0)
                rec["unsafe"] = float(np.nanmax(worst) / THIN)
            elif kind == "vote":
                nth = ngen = 0
                for r0 in range(0, items, threads):
                    for w0 in range(r0, min(items, r0 + threads), WAVE):
                        blk = tl[:, w0:min(items, w0 + WAVE, r0 + threads), :]
                        v = ~(blk > THIN).any(axis=1)
                        nth += int(v.sum())
                        ngen += int((~v).sum())
                rec["votes"] = (nth, ngen)
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.abs(tl / THIN - 1)
            rec["margin"] = float(np.nanmin(np.where(np.isfinite(d), d, np.inf)))
            out.append(rec)
    return plan, out


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def tau_cases():
    cases = []

    def add(name, t, frq, elev, tau, **kw):
        tau = np.array(tau, dtype=np.float64)
        tau[:, 0, :] = 0.0
        cases.append(Case(name, "tau", t, frq, elev, tau=tau, **kw))
    am3 = rr.airmass(E3).max()

    # regimes along one column
    r = rng_of("tiny_column")
    add("tiny_column", temps(2, 17, rng=r), HATPRO, E3, loguniform(r, 1e-8, 0.9 * TINY / am3, (2, 17, 14)))
    r = rng_of("thin_column")
    add("thin_column", temps(2, 17, rng=r), HATPRO, E3, r.uniform(1.1 * TINY / am3, 0.9 * THIN / am3, (2, 17, 14)))
    g = np.geomspace(0.2, 50.0, 16)
    add("general_column", temps(1, 17), HATPRO, np.array([90.0, 30.0, 4.2]),
        np.stack([np.concatenate([[0.0], np.roll(g, j)]) for j in range(14)], axis=1)[None])
    cyc = np.array([0.01, 0.1, 1.0]) / rr.airmass([42.0])[0]
    add("regime_cycle", temps(1, 10), HATPRO, np.array([90.0, 42.0]),
        (cyc[np.arange(10) % 3][:, None] * (1 + 0.01 * np.arange(14))[None, :])[None])
    add("zeros", temps(1, 9), HATPRO, E3, np.zeros((1, 9, 14)))
    ext = np.zeros((1, 9, 14))
    ext[0, :, 0:4], ext[0, :, 4:8] = 1e-300, 1e-20
    ext[0, :, 8:11], ext[0, 8, 8:11] = 1e-20, 1e3
    ext[0, :, 11:14], ext[0, 1, 11:14] = 1e-300, 1e3
    add("extremes", temps(1, 9), HATPRO, E3, ext)
    huge = np.full((1, 9, 14), 0.1) * (1 + 0.01 * np.arange(14))
    for j in range(14):
        huge[0, 1 + j % 8, j] = 1e6 / am3
    add("huge_path", temps(1, 9), HATPRO, np.array([90.0, 4.2]), huge)

    # thresholds: every lane of the wave holds the same value, one value per level
    vals = mr.around(TINY) + mr.around(THIN) + [0.05]               # 19 values: both parities of the level index meet each
    vals = np.array((vals * 4)[:63])
    add("thresholds_zenith", temps(1, 64), HATPRO, np.array([90.0]), np.tile(np.concatenate([[0.0], vals])[None, :, None], (1, 1, 14)))
    e9 = np.array([90.0, 60.0, 45.0, 30.0, 20.0, 15.0, 10.0, 7.0, 5.0])
    a9 = rr.airmass(e9)
    tg = np.concatenate([[0.0], np.where(np.arange(63) % 2 == 0, vals / a9[4], vals / a9[8])])
    add("thresholds_groups", temps(1, 64), HATPRO, e9, np.tile(tg[None, :, None], (1, 1, 14)))

    # one odd lane
    def odd(nf, lanes):
        col = 1 + 1e-3 * np.arange(nf)
        tau = np.empty((2, 9, nf))
        tau[0] = (1e-4 / am3) * col
        tau[1] = 1.0 * col
        for j in lanes:
            tau[0, :, j], tau[1, :, j] = 1.0 * col[j], (1e-4 / am3) * col[j]
        return tau
    f257, f63 = np.linspace(20.0, 60.0, 257), np.linspace(20.0, 60.0, 63)
    add("odd_lane_257", temps(2, 9), f257, E3, odd(257, (0, 127)))
    add("odd_lane_257_base", temps(2, 9), f257, E3, odd(257, ()))
    add("odd_lane_63", temps(2, 9), f63, E3, odd(63, (62,)))
    add("odd_lane_63_base", temps(2, 9), f63, E3, odd(63, ()))

    # per-elevation vote inside the general branch: thin at 90 degrees, general at 4.2
    pe = np.full((1, 9, 14), 0.05) * (1 + 0.01 * np.arange(14))
    pe[0, 3], pe[0, 6] = 1e-4, 0.5
    add("per_elevation_vote", temps(1, 9), HATPRO, E7, pe)

    # the cosmic cut: path totals at zenith (columns 0-6) and through the air mass of 30 degrees (columns 7-13)
    totals = np.array([124.0, 125.0 - 1e-9, 125.0 + 1e-9, 126.0, 200.0, 800.0, 1e5])
    am30 = rr.airmass([30.0])[0]
    cut = np.zeros((1, 9, 14))
    cut[0, 1:, :7] = totals / 8
    cut[0, 1:, 7:] = totals / am30 / 8
    add("cosmic_cut", temps(1, 9), HATPRO, np.array([90.0, 30.0]), cut)

    # Planck votes
    r = rng_of("planck")
    add("planck_split_wave", np.linspace(150.0, 330.0, 10)[None], np.geomspace(100.0, 1000.0, 64), E3, loguniform(r, 1e-3, 0.3, (1, 10, 64)))
    add("planck_along_column", (np.where(np.arange(17) % 2 == 0, 150.0, 160.0) + 0.1 * np.arange(17))[None], np.linspace(99.0, 100.0, 14),
        np.array([90.0]), loguniform(r, 1e-3, 0.3, (1, 17, 14)))
    add("planck_low_x", np.array([[330.0, 329.0]]), np.array([1.0]), np.array([90.0]), np.full((1, 2, 1), 0.01))

    # level and frequency seams; every other one with a wider pitch whose scratch columns hold NaN
    for nlev, nf, nang, extra in ((2, 63, 3, 16), (9, 64, 7, 0), (10, 65, 3, 32), (17, 256, 1, 0), (257, 257, 3, 16), (1024, 65, 1, 0)):
        r = rng_of("seam%d" % nlev)
        elev = {1: np.array([90.0]), 3: E3, 7: E7}[nang]
        add("seam_L%d_F%d" % (nlev, nf), temps(1, nlev, rng=r), np.geomspace(1.0, 1000.0, nf) if nf > 1 else np.array([1.0]), elev,
            loguniform(r, 1e-4, 0.5, (1, nlev, nf)) * min(1.0, 17.0 / nlev), pitch_extra=extra)

    # elevation groups, and one NaN elevation in a group whose longest path is another angle
    r = rng_of("groups")
    gt, gtau = temps(1, 9, rng=r), loguniform(r, 1e-3, 0.5, (1, 9, 14))
    for nang, inan in ((9, 1), (10, 3), (11, 9)):
        elev = np.linspace(88.0, 8.0, nang)
        add("groups_%d" % nang, gt, HATPRO, elev, gtau)
        elev = elev.copy()
        elev[inan] = np.nan
        add("groups_%d_nan" % nang, gt, HATPRO, elev, gtau)

    # flags and confinement
    r = rng_of("flags")
    ft, ftau = temps(4, 9, rng=r), loguniform(r, 1e-3, 0.5, (4, 9, 14))
    add("flags_base", ft, HATPRO, E3, ftau)
    add("flags", ft, HATPRO, E3, ftau, valid=[1, 0, 2, 1])
    nt, ntau = temps(2, 9, rng=r), r.uniform(0.5, 2.0, (2, 9, 14))
    add("nan_tau_base", nt, HATPRO, E3, ntau)
    for name, v, held in (("nan_tau", np.nan, True), ("inf_tau", np.inf, False)):
        bad = ntau.copy()
        bad[0, 4, 5] = v
        add(name, nt, HATPRO, E3, bad, held=held)
    # ... and among tiny lanes, where a NaN lane that voted for the costly branch would move the whole wave (and its bits)
    tt = loguniform(r, 1e-8, 0.9 * TINY / am3, (2, 9, 14))
    add("nan_tau_tiny_base", nt, HATPRO, E3, tt)
    bad = tt.copy()
    bad[0, 4, 5] = np.nan
    add("nan_tau_tiny", nt, HATPRO, E3, bad)
    ng = np.full((1, 9, 14), 0.05) * (1 + 0.01 * np.arange(14))
    ng[0, 4] = -1e-3
    add("negative_tau", temps(1, 9), HATPRO, E3, ng)

    # exact properties
    r = rng_of("batch")
    bt, btau = temps(16, 9, rng=r), loguniform(r, 1e-4, 2.0, (16, 9, 14))
    bt[11], btau[11] = bt[3], btau[3]
    add("batch_neighbours", bt, HATPRO, E3, btau)
    dt = temps(1, 9, rng=r)
    dtau = np.concatenate([loguniform(r, 1e-6, 1e-4, (9, 5)), r.uniform(2e-3, 8e-3, (9, 5)), r.uniform(0.2, 3.0, (9, 4))], axis=1)[None]
    add("dup_base", dt, HATPRO, E3, dtau)
    add("dup_inserted", np.insert(dt, 5, dt[:, 5], axis=1), HATPRO, E3, np.insert(dtau, 6, 0.0, axis=1))
    return cases


def alpha_case(name, t, frq, elev, a, dz, **kw):
    """constant coefficient a [nprof][nf] (all of it in the wet half), thickness dz [nprof][nlev-1]"""
    a, dz = np.asarray(a, dtype=np.float64), np.asarray(dz, dtype=np.float64)
    z = np.concatenate([np.zeros((dz.shape[0], 1)), np.cumsum(dz, axis=1)], axis=1)
    awet = np.repeat(a[:, :, None], z.shape[1], axis=2)
    return Case(name, "alpha", t, frq, elev, awet=awet, adry=np.zeros_like(awet), z=z, **kw)


def seam_positions(nlev, nf, nang):
    """layers (1-based level index) at the first and last layer of every segment of pass 0, the last real layer and the last
    layer of the segment before the last"""
    nseg, seglen, _ = alpha_plan(nlev, nf, nang)["passes"][0]
    pos = []
    for s in range(nseg):
        pos += [1 + s * seglen, min(nlev - 1, (s + 1) * seglen)]
    return sorted(set(pos + [nlev - 1, (nseg - 1) * seglen]))


def alpha_cases():
    cases = []
    am3 = rr.airmass(E3).max()
    F16 = np.sort(np.concatenate([HATPRO, [50.3, 60.0]]))
    r = rng_of("alpha")
    # every loop of the pass: 180 levels x 14 channels x 3 elevations run sorted, x 7 elevations keep the per-step vote,
    # 17 levels have segments under 16 layers
    dz180 = r.uniform(0.01, 0.02, (2, 179))
    col = 0.5 + 0.5 * np.arange(14) / 13
    cases.append(alpha_case("alpha_sorted_thin", temps(2, 180, rng=r), HATPRO, E3, np.tile(0.9 * THIN / am3 / 0.02 * col, (2, 1)), dz180))
    cases.append(alpha_case("alpha_sorted_general", temps(2, 180, rng=r), HATPRO, E3, np.tile(20.0 * (1 + col), (2, 1)), dz180))
    mixed = np.tile(np.where(np.arange(14) % 2 == 0, 0.9 * THIN / am3 / 0.02, 2.0) * col, (2, 1))
    cases.append(alpha_case("alpha_sorted_mixed", temps(2, 180, rng=r), HATPRO, E3, mixed, dz180))
    cases.append(alpha_case("alpha_vote", temps(2, 180, rng=r), HATPRO, E7, np.tile(np.where(np.arange(14) % 2 == 0, 0.2, 3.0) * col, (2, 1)), dz180))
    cases.append(alpha_case("alpha_short", temps(2, 17, rng=r), HATPRO, E3, np.tile(np.where(np.arange(14) % 2 == 0, 0.2, 30.0) * col, (2, 1)),
                            r.uniform(0.1, 0.2, (2, 16))))
    # the float decision: one layer per column whose tau * airmass sits within 1e-7 of 1/8; the rest far below
    dzf = np.full((1, 179), 1e-4)
    dzf[0, 40] = 1.0
    delta = np.array([-2e-6, -1e-6, -6e-7, -1e-7, -1e-9, 1e-9, 1e-7, 6e-7, 1e-6, -3e-8, 3e-8, -1e-8, 1e-8, 2e-6])
    cases.append(alpha_case("alpha_float_edge", temps(1, 180), HATPRO, E3, (THIN * (1 + delta) / rr.airmass(E3)[np.arange(14) % 3])[None], dzf))
    # segment seams: zero thickness everywhere but one layer, which is opaque (T_seg = 0), leaves T_seg = 1e-60, or is a
    # moderate layer between segments whose T_seg is exactly 1
    pos = seam_positions(180, 14, 3)
    kinds = np.array([1e3, 60 * np.log(10.0), 0.3])
    for k, p0 in enumerate(range(0, len(pos), 16)):                      # one profile per position, at most 16 profiles a case
        mine = pos[p0:p0 + 16]
        dzs = np.zeros((len(mine), 179))
        dzs[np.arange(len(mine)), np.array(mine) - 1] = 1.0
        cases.append(alpha_case("alpha_seams_%d" % k, temps(len(mine), 180, rng=r), HATPRO, E3,
                                np.tile(kinds[np.arange(14) % 3] * (1 + 0.01 * np.arange(14)), (len(mine), 1)), dzs))
    # two-pass chunks with the odd (general) column in the second pass
    for nf, frq in ((14, HATPRO), (16, F16)):
        a = np.full((2, nf), 0.5 * THIN / am3 / 0.02)
        a[:, nf - 2] = 50.0
        cases.append(alpha_case("alpha_two_pass_%d" % nf, temps(2, 65, rng=r), frq, E3, a * (1 + 0.01 * np.arange(nf)), r.uniform(0.01, 0.02, (2, 64))))
    # the layer rule: constant, ratios 1.01, 4 and 1e6 between neighbours, a zero level, and a column that mixes them in one wave
    lev = np.arange(65)
    pat = [np.full(65, 0.3), 0.3 * np.where(lev % 2 == 0, 1.0, 1.01), 0.2 * np.where(lev % 2 == 0, 1.0, 4.0),
           np.where(lev % 2 == 0, 1e-6, 1.0), np.where(lev % 7 == 3, 0.0, 0.25)]
    mix = np.choose(lev // 2 % 5, pat)
    rule_w = np.stack([(pat + [mix])[j % 6] * (1 + 0.01 * j) for j in range(14)])[None]
    rule_d = np.stack([(pat + [mix])[(j + 2) % 6] * 0.5 for j in range(14)])[None]
    zr = np.concatenate([[0.0], np.cumsum(r.uniform(0.03, 0.06, 64))])[None]
    cases.append(Case("alpha_layer_rule", "alpha", temps(1, 65, rng=r), HATPRO, E3, awet=rule_w, adry=rule_d, z=zr))
    # flags: a negative and a NaN coefficient blank their own profile only
    fw, fd = np.tile(rule_w, (4, 1, 1)) * r.uniform(0.9, 1.1, (4, 1, 1)), np.tile(rule_d, (4, 1, 1))
    ft, fz = temps(4, 65, rng=r), np.tile(zr, (4, 1))
    cases.append(Case("alpha_flags_base", "alpha", ft, HATPRO, E3, awet=fw, adry=fd, z=fz))
    bw, bd = fw.copy(), fd.copy()
    bw[1, 9, 33], bd[2, 3, 64] = -1e-3, np.nan
    cases.append(Case("alpha_flags", "alpha", ft, HATPRO, E3, awet=bw, adry=bd, z=fz))
    # the cut, transparent and opaque columns at 7 elevations
    totals = np.array([0.0, 124.0, 125.0 - 1e-9, 125.0 + 1e-9, 126.0, 200.0, 800.0, 1e5, 124.0, 126.0, 200.0, 800.0, 1e5, 0.0])
    scale = np.where(np.arange(14) < 8, 1.0, 1.0 / rr.airmass([4.2])[0])
    cases.append(alpha_case("alpha_cut_7", temps(1, 17), HATPRO, E7, (totals * scale / 16)[None], np.ones((1, 16))))
    return cases


@functools.lru_cache(maxsize=None)
def table():
    cases = tau_cases() + alpha_cases()
    by_name = {c.name: c for c in cases}
    assert len(by_name) == len(cases)
    return by_name


def names(entry=None, held=None):
    return [n for n, c in table().items() if (entry is None or c.entry == entry) and (held is None or c.held == held)]


# exact properties: (label, case a, index into its TB [nprof][nang][nf], case b, index) -- the two selections hold the same bits
def exact_pairs():
    T = table()
    s = slice(None)

    def rows_but(case, bad):
        return np.array([a for a in range(T[case].nang) if a != bad])
    out = [("waves without the odd lane", "odd_lane_257", (s, s, slice(128, 257)), "odd_lane_257_base", (s, s, slice(128, 257))),
           ("same column, other profile index and batch neighbours", "batch_neighbours", (3,), "batch_neighbours", (11,)),
           ("duplicate level (same T, tau = 0)", "dup_inserted", (s,), "dup_base", (s,)),
           ("profiles beside the blanked ones", "flags", ([0, 3],), "flags_base", ([0, 3],)),
           ("alpha: profiles beside the flagged ones", "alpha_flags", ([0, 3],), "alpha_flags_base", ([0, 3],))]
    for nang, inan in ((9, 1), (10, 3), (11, 9)):
        k = rows_but("groups_%d" % nang, inan)
        out.append(("rows beside the NaN elevation, nang = %d" % nang, "groups_%d_nan" % nang, (s, k), "groups_%d" % nang, (s, k)))
    other = np.array([j for j in range(14) if j != 5])
    for bad, base in (("nan_tau", "nan_tau_base"), ("inf_tau", "nan_tau_base"), ("nan_tau_tiny", "nan_tau_tiny_base")):
        out.append(("%s: other frequencies of the profile" % bad, bad, (0, s, other), base, (0, s, other)))
        out.append(("%s: the other profile" % bad, bad, (1,), base, (1,)))
    return out


# the cases that sit ON a switch; every other one keeps MARGIN from them (tests/test_rte_reference.py::test_cases_take_their_routes)
THRESHOLD_CASES = ("thresholds_zenith", "thresholds_groups", "alpha_float_edge")
