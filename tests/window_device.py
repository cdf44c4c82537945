"""The device side of the window geometry table (tests/window_cases.py): one function that runs a case through the windowed
and the every-line kernels and returns every figure tests/test_window_geometry.py holds to a bar and
tools/window_geometry_errors.py records."""
import numpy as np

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
import window_cases as wc
import window_reference as wr

ELEVATIONS = np.array([90.0, 30.0, 5.4])
ORACLE_PROFILE = 1            # the profile whose absorption meets the oracle at every frequency (the one a case may weigh down)
TB_STRIDE = 11


class absorption_mode:
    """set_absorption_mode for one call, the automatic choice restored whatever happens"""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.ctx.set_absorption_mode(self.mode)

    def __exit__(self, *exc):
        self.ctx.set_absorption_mode(0)


def relerr(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0))


def profiles_of(case):
    """three 180-level profiles, sharp-line top levels included; profile 1 weighed down where the case says so"""
    return wc.heavy_ground(pr.synthetic_profiles(3, 5), case.heavy_hpa)


def absorption(ctx, m, P, frq, mode):
    with absorption_mode(ctx, mode):
        return ctx.absorption_batch(m, P["p"], P["t"], P["rh"], frq)


def tb(ctx, m, P, frq, mode):
    with absorption_mode(ctx, mode):
        return ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ELEVATIONS)


def measure(ctx, case, model_name, plan):
    """-> dict: `truncation` (per profile, all levels: wr.plan_truncation, reference only), `win_vs_every` (per profile:
    dry, wet), `win_vs_oracle` / `every_vs_oracle` (profile 1, every frequency, relative), `tb_vs_oracle` [K] (every 11th
    frequency, all profiles), `tb_vs_every` [K], `valid`"""
    from oracle import c_oracle as co, lbl_oracle as lo
    m = sp.get_model(model_name)
    P, frq = profiles_of(case), case.frq
    aw, ad = absorption(ctx, m, P, frq, 2)
    dw, dd = absorption(ctx, m, P, frq, 1)
    i = ORACLE_PROFILE
    ow, od = lo.absorption_profile(m, P["p"][i], P["t"][i], P["rh"][i], frq)
    out = dict(win_vs_oracle=max(relerr(aw[i], ow), relerr(ad[i], od)), every_vs_oracle=max(relerr(dw[i], ow), relerr(dd[i], od)),
               finite=bool(np.isfinite(aw).all() and np.isfinite(ad).all()))
    # (a level that takes a speed-dependent line back evaluates it directly: the plan's figure, which keeps the line's
    # Lorentzians in the far set there, is an upper estimate at those three levels)
    out["truncation"] = [wr.plan_truncation(plan, m, {k: P[k][j] for k in ("p", "t", "rh")}) for j in range(3)]
    out["win_vs_every"] = [dict(dry=relerr(ad[j], dd[j]), wet=relerr(aw[j], dw[j])) for j in range(3)]
    tb_auto, valid = tb(ctx, m, P, frq, 0)
    tb_every, valid1 = tb(ctx, m, P, frq, 1)
    sub = np.arange(0, len(frq), TB_STRIDE)
    dev = 0.0
    for j in range(3):
        ref = co.tb_profile(m, P["z"][j], P["p"][j], P["t"][j], P["rh"][j], frq[sub], ELEVATIONS)["tbtotal"]
        dev = max(dev, float(np.abs(tb_auto[j][:, sub] - ref.reshape(len(ELEVATIONS), len(sub))).max()))
    out.update(tb_vs_oracle=dev, tb_vs_every=float(np.abs(tb_auto - tb_every).max()),
               valid=bool((valid == 1).all() and (valid1 == 1).all()), tb_finite=bool(np.isfinite(tb_auto).all()))
    return out


def refusal(ctx, case, model_name):
    """an ineligible list: -> dict(mode0_is_mode1 (absorption and TB, bit for bit), mode2_code (of the MwrtError the absorption entry raises, or None))"""
    from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError
    m = sp.get_model(model_name)
    P, frq = profiles_of(case), case.frq
    a0, a1 = absorption(ctx, m, P, frq, 0), absorption(ctx, m, P, frq, 1)
    t0, t1 = tb(ctx, m, P, frq, 0), tb(ctx, m, P, frq, 1)
    same = all(np.array_equal(x, y) for x, y in zip(a0 + t0, a1 + t1)) and bool(np.isfinite(t0[0]).all())
    try:                                                   # (the TB entry serves such a list with the fused kernel in any mode)
        absorption(ctx, m, P, frq, 2)
        code = None
    except MwrtError as err:
        code = err.code
    return dict(mode0_is_mode1=same, mode2_code=code)
