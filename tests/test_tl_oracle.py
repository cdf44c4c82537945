"""The exact derivative reference (oracle/tl_oracle.py, torch autograd on the CPU) against the NumPy oracle it restates.

Its values must equal lbl_oracle's to rounding and its derivatives lbl_oracle's central differences wherever those are
not noise; then it can stand in for difference quotients in the device K-matrix tests (test_jacobian_device_edges.py),
with tolerances three to four orders tighter.  No GPU here."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp  # noqa: E402
from oracle import lbl_oracle as lo, tl_oracle as tl  # noqa: E402
from oracle.fuzz_tables import fuzzed_tables  # noqa: E402

FAMILIES = ["R98", "R17", "R20", "R20SD"]
FUZZ = [1, 2, 4, 5]          # between them: both shift modes, both mixing modes, both N2 forms, with and without fdep
CASES = FAMILIES + [f"fuzz{s}" for s in FUZZ]


def tables_and_frq(case):
    """The tables and a frequency list that reaches every branch: the low end, line centres, the 60-GHz band, 999 GHz,
    a point inside the speed-dependent window of an SD line and a pair straddling the 750-GHz cutoff of the 22-GHz line."""
    frq = [2.5, 22.235, 60.3061, 118.7503, 183.31, 999.0, 771.9, 772.6]
    if case.startswith("fuzz"):
        m, sdl = fuzzed_tables(int(case[4:]))
        frq.append(float(m.h2o["fl"][sdl[0]]) + 0.3)
    else:
        m = sp.get_model(case)
        if (m.h2o["w2"] > 0).any():
            frq.append(float(m.h2o["fl"][np.argmax(m.h2o["w2"] > 0)]) + 0.3)
    return m, np.array(frq)


def edge_profile(nlev=30, seed=31):
    """A synthetic profile with a dry level, a dry block and a pair of identical neighbouring levels."""
    P = pr.synthetic_profiles(1, seed, nlev=nlev)
    z, p, t, rh = (P[k][0].copy() for k in ("z", "p", "t", "rh"))
    rh[6] = 0.0
    rh[14:17] = 0.0
    p[9], t[9], rh[9] = p[8], t[8], rh[8]
    return z, p, t, rh


@pytest.mark.parametrize("case", CASES)
def test_values_equal_the_oracle(case):
    m, frq = tables_and_frq(case)
    z, p, t, rh = edge_profile()
    e = lo.vapor(t, rh)[0]
    aw, ad = tl.clearsky_absorption(m, *(torch.tensor(x) for x in (p, t, e)), frq)
    for j, f in enumerate(frq):
        w, d = lo.clearsky_absorption(m, p, t, e, f)
        for got, want in ((aw[j].numpy(), w), (ad[j].numpy(), d)):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (case, f)
    ang = np.array([90.0, 4.2, 179.0])
    ref = lo.tb_cloud_rte(m, z, p, t, rh, frq, ang)["tbtotal"].reshape(len(ang), len(frq))
    tb = tl.tb_rh(m, *(torch.tensor(x) for x in (z, p, t, rh)), frq, ang).numpy()
    assert np.abs(tb - ref).max() <= 1e-12 * np.abs(ref).max(), case


def _smooth_check(got, c, fwd, bwd, what, noise=0.0, mask=None):
    """got: exact derivative row; c, fwd, bwd: central / forward / backward differences.  Points where the one-sided
    differences disagree (a branch inside the +- step) carry no derivative to compare against (the criterion of
    test_jacobian_device.py).  ``noise``: the rounding floor of the quotient itself, ~eps |value| / step (scalar or per point) (it matters
    only where a derivative is tiny beside its value, e.g. the dry term's e-derivative at 999 GHz)."""
    scale = np.abs(c).max()
    noise = np.broadcast_to(noise, np.shape(c))
    if scale == 0.0:
        assert np.abs(got).max() <= max(1e-12, noise.max()), what
        return
    smooth = np.abs(fwd - bwd) <= 1e-4 * scale + 2 * noise
    if mask is not None:
        smooth &= mask
    assert smooth.sum() >= 0.75 * (smooth.size if mask is None else mask.sum()), what
    err = (np.abs(got - c) - noise)[smooth]
    assert err.max() <= 1e-6 * scale, (what, err.max() / scale)


@pytest.mark.parametrize("case", CASES)
def test_absorption_derivatives_equal_oracle_differences(case):
    m, frq = tables_and_frq(case)
    z, p, t, rh = edge_profile()
    e = lo.vapor(t, rh)[0]
    ex = tl.absorption_tl(m, p, t, e, frq)
    for j, f in enumerate(frq):
        def ab(tk, ee):
            return lo.clearsky_absorption(m, p, tk, ee, f)
        base = ab(t, e)
        hT = 1e-3
        up, dn = ab(t + hT, e), ab(t - hT, e)
        for s, name in ((0, "awet"), (1, "adry")):
            _smooth_check(ex[f"d{name}_dt"][j].numpy(), (up[s] - dn[s]) / (2 * hT), (up[s] - base[s]) / hT,
                          (base[s] - dn[s]) / hT, (case, f, name, "T"))
            # e: a relative step for the wet term, an absolute one of 1e-5 of the largest e for the dry term; one-sided
            # where e is smaller than the step (dry levels: the reference's tangent is the right-sided derivative)
            he = np.where(e > 0, 1e-5 * e, 1e-6) if s == 0 else np.full_like(e, 1e-5 * e.max())
            two = e > he
            eu, ed = ab(t, e + he), ab(t, np.where(two, e - he, e))
            fwd = (eu[s] - base[s]) / he
            bwd = np.where(two, (base[s] - ed[s]) / he, fwd)
            c = np.where(two, (eu[s] - ed[s]) / (2 * he), fwd)
            noise = 8 * np.finfo(float).eps * np.abs(base[s]).max() / he.min()
            _smooth_check(ex[f"d{name}_de"][j].numpy(), c, fwd, bwd, (case, f, name, "e"), noise)


@pytest.mark.parametrize("case", FAMILIES + ["fuzz2", "fuzz4"])
def test_k_matrix_equals_oracle_differences(case):
    """dTB/dT (fixed e), dTB/de (fixed T) and dTB/d(layer thickness) against central differences of tb_cloud_rte."""
    m, frq = tables_and_frq(case)
    frq = frq[[1, 2, -1]]
    ang = np.array([90.0, 4.2])
    z, p, t, rh = edge_profile(nlev=20, seed=3)
    e = lo.vapor(t, rh)[0]
    es = lo.vapor(t, np.ones_like(t))[0]
    K = tl.k_matrix(m, z, p, t, e, frq, ang)

    def tb(zz=z, tt=t, ee=e):
        # rh that keeps e at the given value at temperature tt
        rr = np.where(ee > 0, ee / lo.vapor(tt, np.ones_like(tt))[0], 0.0)
        return lo.tb_cloud_rte(m, zz, p, tt, rr, frq, ang)["tbtotal"].reshape(len(ang), len(frq))
    base = tb()
    nlev = len(z)
    # the layer rule's |x1 - x0| < 1e-9 band (identical neighbours, here levels 8 and 9, and the dry block): inside it the exact partials
    # are (1, 0), but any finite step in T or e leaves the band and sees the log-mean's (1/2, 1/2).  The step straddles
    # a branch whose jump (< 1e-9 of absorption) is too small for the one-sided test to notice, so both levels of such a
    # layer are left out here; the device tests compare the convention itself
    band = np.zeros((len(frq), nlev), dtype=bool)
    for j, f in enumerate(frq):
        for x in lo.clearsky_absorption(m, p, t, e, f):
            lay = np.abs(np.diff(x)) < 1e-9                   # (the dry block's 0 -> 0 layers too: an e step leaves it)
            band[j, 1:] |= lay
            band[j, :-1] |= lay
    assert band.any()
    for key, h in (("dtb_dt", 1e-3), ("dtb_de", None), ("dtb_ddz", 1e-5)):
        c, fwd, bwd = (np.zeros((len(ang), len(frq), nlev)) for _ in range(3))
        # the quotient's rounding floor: the oracle's TB carries ~1e-12 relative rounding (the log-mean's x1 - x0 and
        # log(x1 / x0) cancel for nearby levels), which only matters where a row is tiny beside TB / step -- e.g. the
        # e-derivatives at 60 GHz, where the path is opaque
        noise = np.zeros(nlev)
        for l in range(nlev):
            if key == "dtb_ddz" and l == 0:
                continue
            if key == "dtb_dt":
                tp, tm = t.copy(), t.copy(); tp[l] += h; tm[l] -= h
                up, dn, hh = tb(tt=tp), tb(tt=tm), h
            elif key == "dtb_de":
                hh = 1e-4 * e[l]
                ep, em = e.copy(), e.copy(); ep[l] += hh; em[l] -= hh
                if e[l] == 0.0:
                    # a dry level: any e > 0 leaves the layer rule's zero-end branch for the log-mean, which tends to 0
                    # as an end value does (a jump in TB); the partials (1/2, 1/2) of the branch taken have no
                    # difference quotient to meet
                    continue
                up, dn = tb(ee=ep), tb(ee=em)
            else:
                zp, zm = z.copy(), z.copy(); zp[l:] += h; zm[l:] -= h
                up, dn, hh = tb(zz=zp), tb(zz=zm), h
            noise[l] = 1e-12 * base.max() / hh
            c[..., l] = (up - dn) / (2 * hh)
            fwd[..., l] = (up - base) / hh
            bwd[..., l] = (base - dn) / hh
        for a in range(len(ang)):
            for j in range(len(frq)):
                ok = None if key == "dtb_ddz" else ~band[j] & ((e > 0) if key == "dtb_de" else True)
                _smooth_check(K[key][a, j].numpy(), c[a, j], fwd[a, j], bwd[a, j], (case, key, a, j), noise, ok)
    assert np.abs(K["tb"].numpy() - base).max() <= 1e-12 * base.max()


def test_k_matrix_equals_full_graph_autograd():
    """tl.k_matrix joins two autograd stages by the chain rule; one backward through the whole (dz, p, T, e) graph
    must give the same rows."""
    m, frq = tables_and_frq("fuzz2")
    z, p, t, rh = edge_profile(nlev=20, seed=5)
    ang = np.array([30.0, 1.0])
    e = lo.vapor(t, rh)[0]
    K = tl.k_matrix(m, z, p, t, e, frq, ang)
    dz = torch.tensor(np.append(0.0, np.diff(z - z[0])), requires_grad=True)
    tt, et = torch.tensor(t, requires_grad=True), torch.tensor(e, requires_grad=True)
    tb = tl.tb_dz(m, dz, torch.tensor(p), tt, et, frq, ang)
    for a in range(len(ang)):
        for j in range(len(frq)):
            g = torch.autograd.grad(tb[a, j], (tt, et, dz), retain_graph=True)
            for gi, key in zip(g, ("dtb_dt", "dtb_de", "dtb_ddz")):
                want = gi.numpy()
                assert np.abs(K[key][a, j].numpy() - want).max() <= 1e-12 * np.abs(want).max(), (key, a, j)


def zero_thickness_case():
    """A 30-level synthetic R24 profile whose layer 11 (between levels 10 and 11) has zero thickness."""
    P = pr.synthetic_profiles(1, 0, nlev=30)
    z, p, t, rh = (P[k][0].copy() for k in ("z", "p", "t", "rh"))
    z[11:] -= z[11] - z[10]
    return sp.get_model("R24"), z, p, t, rh, np.array([53.86]), np.array([90.0])


def test_zero_thickness_layer_derivative():
    """TB depends on a layer's thickness through tau_l = m L_l dz_l, linear and defined at dz = 0: the derivative there is
    g_l m (Lw + Ld), not 0.  The oracle's difference quotients (central and both one-sided, converging together) pin it."""
    m, z, p, t, rh, frq, ang = zero_thickness_case()
    assert z[11] == z[10]
    K = tl.k_matrix_rh(m, z, p, t, rh, frq, ang)
    got = float(K["dtb_ddz"][0, 0, 11])
    assert abs(got - 9.6415) < 5e-4, got

    def tb(zz):
        return lo.tb_cloud_rte(m, zz, p, t, rh, frq, ang)["tbtotal"][0]
    base = tb(z)
    gaps = []
    for h in (1e-3, 1e-4, 1e-5):
        zp, zm = z.copy(), z.copy(); zp[11:] += h; zm[11:] -= h
        up, dn = tb(zp), tb(zm)
        assert abs((up - dn) / (2 * h) - got) <= 1e-6 * abs(got), h
        gaps.append(abs((up - base) / h - (base - dn) / h))
    assert gaps[0] > gaps[1] > gaps[2]           # the one-sided quotients converge onto the central one
    assert abs((tb(z + np.where(np.arange(30) >= 11, 1e-6, 0.0)) - base) / 1e-6 - got) <= 1e-4 * abs(got)


def test_goff_gratch_derivative_equals_autograd():
    from mwr_fast_forward_operators_and_lbls_amd import autodiff
    t = torch.linspace(150.0, 340.0, 401, dtype=torch.float64, requires_grad=True)
    es, _ = tl.vapor(t, torch.ones_like(t))
    (want,) = torch.autograd.grad(es.sum(), t)
    got_es, got = autodiff.goff_gratch_es(t.detach())
    assert torch.allclose(got_es, es.detach(), rtol=1e-13, atol=0)
    assert ((got - want).abs() <= 1e-12 * want.abs()).all()


@pytest.mark.parametrize("zero_layer", [False, True])
def test_autograd_backward_equals_reference_autograd(monkeypatch, zero_layer):
    """autodiff's backward (contraction + chain rule to z, t, rh) with the native call replaced by the reference K-matrix,
    against the reference's own autograd in z, t and rh."""
    from mwr_fast_forward_operators_and_lbls_amd import autodiff
    m, frq = tables_and_frq("R20SD")
    frq = frq[[1, 2, 4]]
    ang = np.array([90.0, 19.2])
    if zero_layer:
        _, z, p, t, rh, _, _ = zero_thickness_case()
    else:
        z, p, t, rh = edge_profile(nlev=24, seed=13)

    def stand_in(model, z_, p_, t_, rh_, frq_, elev, stream):
        K = tl.k_matrix_rh(m, *(x[0].detach() for x in (z_, p_, t_, rh_)), frq_, elev)
        return (K["tb"][None], torch.ones(1, dtype=torch.uint8), K["dtb_dt"][None], K["dtb_de"][None],
                K["dtb_ddz"][None])
    monkeypatch.setattr(autodiff, "_native_jacobian", stand_in)
    w = np.random.default_rng(7).uniform(-1.0, 1.0, (len(ang), len(frq)))
    xs = [torch.tensor(x[None], requires_grad=True) for x in (z, t, rh)]
    tb, valid = autodiff.brightness_temperature(m, xs[0], torch.tensor(p[None]), xs[1], xs[2], frq, ang)
    (tb[0] * torch.tensor(w)).sum().backward()
    want = tl.direct_gradients(m, z, p, t, rh, frq, ang, weights=w)
    for x, k in zip(xs, ("z", "t", "rh")):
        got, ref = x.grad[0].numpy(), want[k].numpy()
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (k, np.abs(got - ref).max() / np.abs(ref).max())


def test_log_mean_partials_are_accurate_for_close_levels():
    """The reference's log-mean partials against 50-digit decimal arithmetic, from s = 1e-9 (levels nearly equal) to
    s ~ 1: float64 autograd of the quotient itself would lose ~eps / s^2 here."""
    from decimal import Decimal, localcontext
    rng = np.random.default_rng(1)
    x0 = rng.uniform(1e-3, 10.0, 300)
    s = 10.0 ** rng.uniform(-9, 0, 300) * rng.choice([-1.0, 1.0], 300)
    x1 = x0 * (1 + s) / (1 - s)
    a, b = torch.tensor(x1, requires_grad=True), torch.tensor(x0, requires_grad=True)
    tl._LogMean.apply(a, b).sum().backward()
    with localcontext() as ctx:
        ctx.prec = 50
        for i in range(len(x0)):
            A, B = Decimal(x1[i]), Decimal(x0[i])
            ln = (A / B).ln()
            L = (A - B) / ln
            for got, want in ((a.grad[i].item(), float((1 - L / A) / ln)), (b.grad[i].item(), float((L / B - 1) / ln))):
                assert abs(got - want) <= 1e-14 * abs(want), (s[i], got, want)
