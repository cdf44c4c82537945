"""(no GPU) Pins tests/rte_reference.py and tests/rte_cases.py before anything is compared with them: closed forms at 45
digits, the long-double evaluator against the 50-digit one on every column of the table, the double oracle against the
reference under the same bars, the route every case is built for, the bound on the cosmic term at the cut, and a double
emulation of the recursion with switchable defects that the table has to see.

FIGURES (this module prints them): the long-double evaluator meets mpmath to 1.9e-18 relative on the table, where the smallest
bar is 1.8e-14 relative (1e-13 K); the long-double layer rule meets the decimal one to 1.1e-19; each defect of the emulation
misses a bar by 2e8 x or more; lo.planck_down + lo.bright in double miss the bars on 8 cases: see test_the_oracle."""
import functools

import mpmath as mp
import numpy as np
import pytest

import math_reference as mr
import rte_cases as rc
import rte_device as rd
import rte_reference as rr

C = rr.model_consts()
mp45 = mp.mpf(10) ** -45


def planck_mp(f, tk):
    hvk = mp.mpf(float(f)) * mp.mpf(10) ** 9 * mp.mpf(C.planck_h) / mp.mpf(C.boltzmann_k)
    return 1 / (mp.exp(hvk / mp.mpf(float(tk))) - 1), hvk


FREQS = sorted({float(f) for c in rc.table().values() for f in c.frq})


def test_long_double_is_wide_enough():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_closed_form_isothermal():
    """B = b(T)(1 - e^-S) + b(t_c) e^-S for an isothermal column, whatever the split into layers"""
    with mp.workdps(50):
        for f in (1.0, 22.24, 58.0, 183.31, 1000.0):
            for split in ([3.0], [1.0, 2.0], [0.5] * 6, [1e-3, 2.9, 0.099], [2.0 ** -k for k in range(1, 12)] + [3 - 1 + 2.0 ** -11]):
                for am in (1.0, 2.5):
                    S = sum(mp.mpf(s) for s in split) * mp.mpf(am)
                    bT, hvk = planck_mp(f, 250.0)
                    want = bT * (1 - mp.exp(-S)) + planck_mp(f, C.t_cosmic)[0] * mp.exp(-S)
                    tb, B, _, _ = rr.evaluate_mp([0.0] + split, [250.0] * (len(split) + 1), f, [am], C)[0]
                    assert abs(B / want - 1) < mp45 and abs(tb / (hvk / mp.log(1 + 1 / want)) - 1) < mp45


def test_transparent_column_gives_t_cosmic():
    with mp.workdps(50):
        for f in FREQS:
            tb = rr.evaluate_mp([0.0] * 5, [290.0, 280.0, 270.0, 260.0, 250.0], f, [1.0, 13.0], C)
            assert all(abs(r[0] / mp.mpf(C.t_cosmic) - 1) < mp45 for r in tb), f


def test_opaque_first_layer():
    """tau_1 -> inf: E = 0, so B = b_0 (the mean (b_0 + b_1 E)/(1 + E) of levels 0 and 1 with the weight of level 1 gone),
    and to first order in E: B = b_0 + E (b_1 - 2 b_0) + O(E^2), written out by hand"""
    with mp.workdps(50):
        for f in (22.24, 58.0, 340.0):
            b0, hvk = planck_mp(f, 290.0)
            b1 = planck_mp(f, 270.0)[0]
            tb, B, cosmic, _ = rr.evaluate_mp([0.0, 1e5, 0.3], [290.0, 270.0, 250.0], f, [1.0], C)[0]
            assert cosmic == 0 and abs(B / b0 - 1) < mp45 and abs(tb / (hvk / mp.log(1 + 1 / b0)) - 1) < mp45
            tau = 20.0
            E = mp.exp(-mp.mpf(tau))
            _, B, _, _ = rr.evaluate_mp([0.0, tau], [290.0, 270.0], f, [1.0], C)[0]
            by_hand = (b0 + b1 * E) / (1 + E) * (1 - E) + planck_mp(f, C.t_cosmic)[0] * E
            assert abs(B / by_hand - 1) < mp45
            assert abs(B - (b0 + E * (b1 - 2 * b0 + planck_mp(f, C.t_cosmic)[0]))) < 10 * E * E * b0


def test_slant_path_is_zenith_of_scaled_tau():
    """a column at air mass am equals the column with tau * am at zenith (the products taken exactly)"""
    with mp.workdps(50):
        tau, t = [0.0, 0.01, 0.5, 2.0, 1e-7], [290.0, 280.0, 265.0, 240.0, 220.0]
        for e in (30.0, 4.2):
            am = rr.airmass([e])[0]
            a = rr.evaluate_mp(tau, t, 31.4, [am], C)[0]
            b = rr.evaluate_mp([mp.mpf(v) * mp.mpf(am) for v in tau], t, 31.4, [1.0], C)[0]
            assert abs(a[0] / b[0] - 1) < mp45


@functools.lru_cache(maxsize=None)
def mp_columns(name):
    """every column of a case at 50 digits: (TB as longdouble [nprof][nang][nf], B, the cosmic term / B at the cut's neighbours)"""
    case = rc.table()[name]
    skip = case.nan_expected()
    tb = np.full((case.nprof, case.nang, case.nf), np.nan, dtype=rr.LD)
    with mp.workdps(50):
        if case.entry == "alpha":
            dz = rr.layer_dz(case.z)
        for p in range(case.nprof):
            for j in range(case.nf):
                if skip[p, :, j].all():
                    continue
                if case.entry == "tau":
                    col = case.tau[p, :, j]
                else:
                    with mr.decimal.localcontext() as ctx:
                        ctx.prec = mr.PREC
                        lw = mr.ref_layer(case.awet[p, j, 1:], case.awet[p, j, :-1])
                        ld = mr.ref_layer(case.adry[p, j, 1:], case.adry[p, j, :-1])
                    col = [mp.mpf(0)] + [(mp.mpf(str(w[1])) + mp.mpf(str(d[1]))) * mp.mpf(float(dz[p, i + 1])) for i, (w, d) in enumerate(zip(lw, ld))]
                ams = [a for k, a in enumerate(case.am) if not skip[p, k, j]]
                res = rr.evaluate_mp(col, case.t[p], case.frq[j], ams, C)
                for k, r in zip([k for k in range(case.nang) if not skip[p, k, j]], res):
                    tb[p, k, j] = rr.mp_to_ld(r[0])
    return tb


@pytest.mark.parametrize("name", rc.names(held=True))
def test_the_two_evaluators_agree(name):
    """no case has more than 4096 columns: every column of every case goes through mpmath"""
    case = rc.table()[name]
    assert case.nprof * case.nang * case.nf <= 4096
    ref = case.reference
    keep = ~case.nan_expected()
    rel = np.abs(ref["tb"][keep] / mp_columns(name)[keep] - 1).astype(np.float64)
    smallest_bar = float((ref["bar"][keep] / np.abs(ref["tb"][keep]).astype(np.float64)).min())
    print("%-24s %5d columns: long double vs 50 digits, worst relative difference %.2e; smallest bar %.2e relative" % (name, keep.sum(), rel.max(), smallest_bar))
    assert np.isfinite(rel).all() and rel.max() * 100 <= smallest_bar


def test_bars_are_where_the_derivation_puts_them():
    """4e-12 K (fdiv1 at 300 K) up to 3e-10 K, except where a 1-GHz lane shares its Planck vote with lanes above 1/32: the general
    branch's exp(x) - 1 at x = 1.5e-4 costs 4e-16 / x = 5e-12 relative, 1.6e-9 K -- the one term that takes a bar above 1e-9 K"""
    over = {}
    for name in rc.names(held=True):
        case = rc.table()[name]
        bar = case.reference["bar"][~case.nan_expected()]
        assert bar.min() > 1e-13 and bar.max() < 2e-9, (name, bar.min(), bar.max())
        if bar.max() > 1e-9:
            over[name] = float(bar.max())
    assert set(over) <= {"seam_L2_F63", "seam_L9_F64", "seam_L10_F65", "seam_L1024_F65"}, over
    for name in over:                                    # ... each of them a column below 2 GHz in a wave that votes general
        case = rc.table()[name]
        where = np.argwhere(case.reference["bar"] > 1e-9)
        assert (case.frq[where[:, 2]] < 2.0).all(), name


@pytest.mark.parametrize("name", rc.names(held=True))
def test_the_oracle(name):
    """lo.planck_down + lo.bright in double, held to the bars the device is held to.  FINDING: it misses them on the
    cases of ORACLE_MISSES, by up to 1.24 x on seven and 3.4 x on the 1-GHz column.  Its Planck function is 1 / (np.exp(x) - 1): the
    subtraction costs eps / (2 x) relative, 3e-14 at 22 GHz and 290 K (9e-12 K) and 8e-13 at 1 GHz (1.2e-12 K where the bar,
    with the kernels' Bernoulli series, is 3.5e-13 K).  The kernels meet every bar (tests/test_rte_columns.py); the oracle
    stays as it is -- pyrtlib's own arithmetic -- and these figures are the floor of any comparison with it."""
    case = rc.table()[name]
    row = rd.check_case(name, rd.oracle_tb(case), case.valid_expected, label="oracle " + name)[0]
    if name in ORACLE_MISSES:
        assert 1.0 < row["worst_err_over_bar"] <= ORACLE_MISSES[name], "the oracle's figure moved: correct the list"
    else:
        assert row["worst_err_over_bar"] <= 1.0, row


# largest error / bar the oracle may show where it misses (measured 1.004 .. 1.234 and 3.371; a tenth of headroom)
ORACLE_MISSES = {"alpha_cut_7": 1.1, "batch_neighbours": 1.1, "odd_lane_63": 1.15, "odd_lane_63_base": 1.15, "odd_lane_257": 1.15,
                 "odd_lane_257_base": 1.15, "seam_L17_F256": 1.35, "planck_low_x": 3.7}


def test_cases_take_their_routes():
    T = rc.table()
    for name, case in T.items():
        if case.entry == "tau":
            _, margin = rc.tau_votes(case)
        else:
            margin = min(r["margin"] for r in rc.alpha_routes(case)[1])
        assert name in rc.THRESHOLD_CASES or margin >= rc.MARGIN, (name, margin)
        assert case.nprof <= 16 and case.nlev in (2, 3, 9, 10, 17, 64, 65, 180, 257, 1024) and case.nang in (1, 2, 3, 7, 9, 10, 11), name

    def steps(name, g=0):
        return rc.tau_votes(T[name])[0][g]["step"]
    assert (steps("tiny_column") == 0).all() and (steps("thin_column") == 1).all() and (steps("general_column") == 2).all()
    assert (steps("regime_cycle")[0, 0] == np.arange(1, 10) % 3).all()
    assert (steps("zeros") == 0).all()
    assert (steps("huge_path") == 2).all() and (np.abs(T["huge_path"].tau).max() * T["huge_path"].am.max() == pytest.approx(1e6))
    # thresholds: at zenith the product IS the listed double; each switch is met exactly, from below and from above
    z = steps("thresholds_zenith")[0, 0]
    v = T["thresholds_zenith"].tau[0, 1:, 0]
    for thr, below, above in ((rc.TINY, 0, 1), (rc.THIN, 1, 2)):
        assert (z[v == thr] == below).all() and (v == thr).any()
        assert (z[v == np.nextafter(thr, 1)] == above).all() and (z[v == np.nextafter(thr, 0)] == below).all()
    g0, g1 = steps("thresholds_groups", 0)[0, 0], steps("thresholds_groups", 1)[0, 0]
    assert set(g0) == {0, 1, 2} and set(g1) == {0, 1, 2} and (g0 != g1).sum() >= 20       # the same level, another longest path
    # one odd lane moves its wave: waves 0 and 1 of the 257 case against the base, waves 2 - 4 untouched
    o, b = steps("odd_lane_257"), steps("odd_lane_257_base")
    assert (o[0, :2] == 2).all() and (b[0, :2] == 0).all() and (o[:, 2:] == b[:, 2:]).all()
    assert (o[1, :2] == 2).all() and (b[1, :2] == 2).all()                                 # a tiny lane among general ones: stays general
    assert (steps("odd_lane_63")[0] == 2).all() and (steps("odd_lane_63_base")[0] == 0).all()
    pe = rc.tau_votes(T["per_elevation_vote"])[0][0]
    mixed = pe["elev_thin"][0, 0][pe["step"][0, 0] == 2]
    assert (mixed[:, 0] & ~mixed[:, -1]).sum() >= 5 and not mixed[:, -1].any()                                 # thin at 90 degrees, general at 4.2
    # a NaN lane votes for the cheap branches: the wave's vote is that of the base
    assert (steps("nan_tau") == steps("nan_tau_base")).all() and (steps("nan_tau") == 2).all()
    assert (steps("nan_tau_tiny") == 0).all() and (steps("nan_tau_tiny_base") == 0).all()
    # Planck votes
    c = T["planck_split_wave"]
    x = 1e9 * C.planck_h / C.boltzmann_k * c.frq[None, :] / c.t[0][:, None]
    assert ((x > mr.PLANCK_SMALL_X).any(axis=1) & (x <= mr.PLANCK_SMALL_X).any(axis=1)).sum() >= 3
    c = T["planck_along_column"]
    x = 1e9 * C.planck_h / C.boltzmann_k * c.frq[None, :] / c.t[0][:, None]
    general = (x > mr.PLANCK_SMALL_X).any(axis=1)
    assert (general[::2]).all() and not general[1::2].any()
    assert 1e9 * C.planck_h / C.boltzmann_k * 1.0 / 330.0 < 1e-3 and T["planck_low_x"].nlev == 2 and T["planck_low_x"].nf == 1
    # seams
    assert {T[n].nlev for n in T if n.startswith("seam")} | {2} == {2, 9, 10, 17, 257, 1024}
    assert {T[n].nf for n in T if T[n].entry == "tau"} >= {1, 14, 63, 64, 65, 256, 257}
    assert {T[n].pitch_extra for n in T if n.startswith("seam")} == {0, 16, 32}
    for nang, groups in ((9, [(0, 5), (5, 4)]), (10, [(0, 10)]), (11, [(0, 8), (8, 3)])):
        assert rc.angle_groups(nang) == groups
        c = T["groups_%d_nan" % nang]
        k = int(np.flatnonzero(np.isnan(c.elev))[0])
        a0, na = next(g for g in groups if g[0] <= k < g[0] + g[1])
        assert np.nanargmax(c.am[a0:a0 + na]) + a0 != k and len(set(T["groups_%d" % nang].elev)) == nang


def test_alpha_cases_take_their_loops():
    T = rc.table()
    # the thread count and the fourth wave of the from-absorption launch; the passes of the 180-level shapes
    assert rc.alpha_plan(180, 14, 3) == dict(threads=256, nfc=14, passes=[(10, 18, 8), (14, 13, 6)], ld=181, kinds=["sorted", "short"])
    assert rc.alpha_plan(180, 14, 7)["kinds"] == ["vote", "sorted"] and rc.alpha_plan(180, 14, 1)["threads"] == 192
    assert rc.alpha_plan(65, 16, 3)["nfc"] == 16 and [p[2] for p in rc.alpha_plan(65, 16, 3)["passes"]] == [8, 8]
    assert [p[2] for p in rc.alpha_plan(65, 14, 3)["passes"]] == [8, 6]

    def routes(name):
        return rc.alpha_routes(T[name])[1]
    assert all(l == {"thin"} for l in routes("alpha_sorted_thin")[0]["loops"])
    assert all(l == {"general"} for l in routes("alpha_sorted_general")[0]["loops"])
    assert all("mixed" in l and "thin" in l for l in routes("alpha_sorted_mixed")[0]["loops"])
    v = routes("alpha_vote")
    assert v[0]["kind"] == "vote" and min(v[0]["votes"]) > 0 and all({"thin", "general"} <= l for l in v[1]["loops"])
    s = routes("alpha_short")
    assert [r["kind"] for r in s] == ["vote", "vote"] and s[0]["seglen"] < rc.K2_SORT_MIN_SEGLEN
    assert {r["kind"] for n in ("alpha_two_pass_14", "alpha_two_pass_16", "alpha_layer_rule") for r in routes(n)} == {"short", "vote"}
    seen = {r["kind"] for n in rc.names("alpha") for r in routes(n)}
    assert seen == {"sorted", "vote", "short"}
    for n in rc.names("alpha"):
        for r in routes(n):
            if r["kind"] == "sorted":
                assert r["unsafe"] <= 1.0, (n, r["unsafe"])                      # no item in the thin loop holds a layer above 1/8
                assert n == "alpha_float_edge" or r["float_margin"] >= rc.FLOAT_MARGIN, (n, r["float_margin"])
    # the float decision: columns within 1e-6 of 1/8 on both sides; the guard sends those within 4e-7 below it to the general loop
    e = routes("alpha_float_edge")[0]
    c = T["alpha_float_edge"]
    tl = np.asarray(c.tau_ld, dtype=np.float64)[0, 41, :8] * c.am[np.arange(8) % 3]
    assert (np.abs(tl / rc.THIN - 1) <= 2.1e-6).all() and (tl > rc.THIN).sum() >= 3 and (tl < rc.THIN).sum() >= 4
    assert e["unsafe"] > 1 - 3e-6 and e["float_margin"] < 1e-6
    # two-pass chunks: the odd (general) column sits in the second pass
    for nf in (14, 16):
        c = T["alpha_two_pass_%d" % nf]
        assert np.argmax(c.awet[0, :, 0]) >= rc.NFK
    # seams: every first and last layer of every segment of pass 0, the last real layer, and T_seg in {0, 1, 1e-60}
    pos = set(rc.seam_positions(180, 14, 3))
    got = set()
    for n in rc.names("alpha"):
        if n.startswith("alpha_seams"):
            c = T[n]
            got |= {int(i) for i in np.flatnonzero((rr.layer_dz(c.z) > 0).any(axis=0))}
            t = np.asarray(c.reference["T"], dtype=np.float64)[:, 0, :3]                  # zenith: opaque, 1e-60, moderate
            assert (t[:, 0] == 0).all() and ((t[:, 1] > 1e-62) & (t[:, 1] < 2e-60)).all() and (t[:, 2] > 0.7).all()
    assert got == pos and {1, 18, 19, 162, 163, 179} <= pos
    # the layer rule: every branch, and one wave that mixes them
    c = T["alpha_layer_rule"]
    br = {mr.layer_branch(a, b) for x in (c.awet, c.adry) for j in range(14) for a, b in zip(x[0, j, 1:], x[0, j, :-1])}
    assert br == {"same", "zero", "small", "mid", "any"}
    assert len({mr.layer_branch(a, b) for a, b in zip(c.awet[0, 5, 1:], c.awet[0, 5, :-1])}) >= 4
    assert list(T["alpha_flags"].valid_expected) == [1, 2, 0, 1]


def test_layer_values_meet_the_decimal_rule():
    """rte_reference.layer_value_ld against math_reference.ref_layer (50 digits) on the layer-rule case"""
    c = rc.table()["alpha_layer_rule"]
    worst = 0.0
    for x in (c.awet, c.adry):
        v, _ = rr.layer_value_ld(x[0, :, 1:], x[0, :, :-1])
        for j in range(c.nf):
            ref = mr.ref_layer(x[0, j, 1:], x[0, j, :-1])
            for i, r in enumerate(ref):
                want = float(r[1])
                got = v[j, i]
                assert (got == 0) if want == 0 else abs(float(got / rr.LD(want) - 1)) < 1e-15
                if want:
                    hi = rr.LD(want) + rr.LD(float(r[1] - mr.D(want)))
                    worst = max(worst, abs(float(got / hi - 1)))
    print("layer rule in long double vs decimal: %.2e relative" % worst)
    assert worst < 1e-18


def test_cosmic_term_at_the_cut_is_below_1e50_of_B():
    """the reference adds the term where sum tl < 125, the kernels where T > exp(-125): within 1e-6 of the cut either may
    happen, and there the term is below 1e-50 of B; away from it the two rules agree (T in double against TRANS_MIN)"""
    seen = 0
    for name in rc.names(held=True):
        case = rc.table()[name]
        ref = case.reference
        keep = ~case.nan_expected()
        near = ref["near_cut"] & keep
        seen += int(near.sum())
        if near.any():
            assert float((ref["bbgT"][near] / ref["B"][near]).max()) < 1e-50, name
        away = keep & ~ref["near_cut"]
        assert ((np.asarray(ref["T"], dtype=np.float64)[away] > rr.TRANS_MIN) == (ref["tauprof"][away] < rr.TAUMAX)).all(), name
    assert seen >= 6                                       # 125 -+ 1e-9 at zenith and through the air mass, both entries


# ---------------------------------------------------------------------------------------------------------------------
# a double emulation of the recursion with switchable defects: the table has to see each of them
# ---------------------------------------------------------------------------------------------------------------------
def emulate(case, defect=None):
    """plain NumPy in double: the recursion per launch group (tau entry) or per pass and segment with the serial
    recombination (alpha entry).  Not the device's arithmetic -- the same formulas at the same precision."""
    tau = np.asarray(case.tau_ld, dtype=np.float64).copy()
    P, L, F = tau.shape
    hvk = case.frq * 1e9 * C.planck_h / C.boltzmann_k
    with np.errstate(all="ignore"):
        b = 1.0 / np.expm1(hvk[None, None, :] / case.t[:, :, None])
        bbg = 1.0 / np.expm1(hvk / C.t_cosmic)
        if defect == "neighbour_column" and F > 6:
            tau[:, :, 5] = tau[:, :, 6]
        if defect == "shadow_live" and F > 1:
            tau[:, :, F - 2] = tau[:, :, F - 1]
        if case.entry == "tau":
            seglen = np.full(F, L - 1)
        else:
            plan = rc.alpha_plan(case.nlev, case.nf, case.nang)
            seglen = np.array([plan["passes"][(j % plan["nfc"]) // rc.NFK][1] for j in range(F)])
        am = case.am.copy()
        if defect == "a0_ignored" and case.entry == "tau":
            for a0, na in rc.angle_groups(case.nang):
                am[a0:a0 + na] = case.am[:na]
        shape = (P, case.nang, F)
        B, T = np.zeros(shape), np.ones(shape)
        Bs, Ts = np.zeros(shape), np.ones(shape)
        nfold = np.zeros(F, dtype=int)
        for i in range(1, L + 1):
            fold = ((i - 1) % seglen == 0) & (i > 1) if i < L else np.ones(F, dtype=bool)
            if fold.any():                                           # B = B + T B_seg, T *= T_seg, in segment order
                drop = defect == "segment_T_dropped"
                Bn = B + T * Bs
                Tn = np.where((nfold == 0)[None, None, :] & drop & (i < L), T, T * Ts)
                B, T = np.where(fold, Bn, B), np.where(fold, Tn, T)
                Bs, Ts = np.where(fold, 0.0, Bs), np.where(fold, 1.0, Ts)
                nfold += fold
            if i == L:
                break
            tl = tau[:, i, None, :] * am[None, :, None]
            E = np.exp(-tl)
            bp = b[:, i if defect == "bprev_wrong_level" else i - 1, None, :]
            bi = b[:, i, None, :]
            th = -np.expm1(-tl) / (1.0 + E)
            if defect == "half_tl_for_tanh":
                th = np.where(np.abs(tl) <= rc.THIN, 0.5 * tl, th)
            if defect == "thin_above_switch_truncated":
                x = -tl
                Et = 1 + x * (1 + x / 2 * (1 + x / 3 * (1 + x / 4 * (1 + x / 5 * (1 + x / 6 * (1 + x / 7 * (1 + x / 8)))))))
                u = tl * tl
                tht = tl * (0.5 - u / 24 + u * u / 240)
                sel = (np.abs(tl) > rc.THIN) & (np.abs(tl) <= 0.5)
                E, th = np.where(sel, Et, E), np.where(sel, tht, th)
            Bs = Bs + (bp + bi * E) * Ts * th
            Ts = Ts * E
        tauprof = (tau[:, 1:, None, :] * am[None, None, :, None]).sum(axis=1)
        add = np.ones(shape, dtype=bool) if defect == "cosmic_past_cut" else (T > rr.TRANS_MIN)
        Btot = np.where(add, B + bbg[None, None, :] * T, B)
        tb = hvk[None, None, :] / np.log(1.0 + 1.0 / Btot)
    tb[case.nan_expected()] = np.nan
    return tb


def emulation_over_bar(name, defect):
    case = rc.table()[name]
    ref = case.reference
    keep = ~case.nan_expected()
    err = np.abs(emulate(case, defect)[keep].astype(rr.LD) - ref["tb"][keep])
    return float((err / ref["bar"][keep]).max())


def test_emulation_without_defect_meets_every_bar():
    for name in rc.names(held=True):
        worst = emulation_over_bar(name, None)
        assert worst <= 1.0, (name, worst)


DEFECT_SEEN_BY = {"bprev_wrong_level": "general_column", "half_tl_for_tanh": "thin_column", "thin_above_switch_truncated": "per_elevation_vote",
                  "segment_T_dropped": "alpha_seams_0", "neighbour_column": "odd_lane_257", "shadow_live": "odd_lane_63",
                  "a0_ignored": "groups_9"}


@pytest.mark.parametrize("defect", sorted(DEFECT_SEEN_BY))
def test_the_table_sees_each_defect(defect):
    name = DEFECT_SEEN_BY[defect]
    worst = emulation_over_bar(name, defect)
    print("%-30s %-22s error / bar %.3g" % (defect, name, worst))
    assert worst >= 100.0, (defect, name, worst)


def test_cosmic_term_past_the_cut_cannot_be_seen():
    """the eighth defect of the list -- the cosmic term added past the cut while T is not yet 0 -- changes B by less than
    1e-50 of itself (the bound asserted above): no bar can see it, and no case is named for it.  What the table does pin is
    that the emulation with that defect still meets every bar, i.e. the cut is not where an error could hide."""
    for name in ("cosmic_cut", "alpha_cut_7"):
        assert emulation_over_bar(name, "cosmic_past_cut") <= 1.0
