"""The device side of the helper tests: each function runs one helper through ``Context.selftest_helpers`` on the input set
of tests/math_reference.py and holds it to that module's reference and bar.  tests/test_math_helpers.py asserts on the
rows these return; tools/math_helper_errors.py writes them to profiles/math_helper_errors.json."""
import functools

import numpy as np

import math_reference as mr

EPS = mr.EPS


def run(ctx, helper, ins, block=mr.BLOCK):
    return ctx.selftest_helpers(helper, ins, block=block)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the references of the scalar helpers, computed once per process"""
    x = mr.inputs({"planck_b_bernoulli": "planck_bernoulli", "planck_b_general": "planck_general", "hui": "hui_w_dw"}.get(name, name))
    if name in ("fexp_small", "fexp_tiny"):
        return mr.ref_exp(x[0])
    if name in ("ftanh_half_small", "ftanh_half_tiny"):
        return mr.ref_tanh_half(x[0])
    if name == "two_atanh_tail":
        return mr.ref_two_atanh_over_s(x[0])
    if name == "fsqrt":
        return mr.ref_sqrt(x[0])
    if name == "crecip":
        return mr.ref_crecip(*x)
    if name == "cmul_cdiv":
        return mr.ref_cmul_cdiv(*x)
    if name == "csqrt_principal":
        return mr.ref_csqrt(*x)
    if name == "hui":
        return mr.ref_hui(*mr.inputs("hui_w_dw"))
    if name in ("planck_b_bernoulli", "planck_b_general"):
        return mr.ref_planck(x[0])
    raise KeyError(name)


def layer_reference(zeroflg):
    return _layer_reference(bool(zeroflg))


@functools.lru_cache(maxsize=None)
def _layer_reference(zeroflg):
    x1, x0, _ = mr.inputs("layer")
    return mr.ref_layer(x1, x0, zeroflg)


@functools.lru_cache(maxsize=None)
def layer_waves(lanes_per_thread):
    x1, x0, live = mr.inputs("layer")
    return mr.wave_branches(x1, x0, live, lanes_per_thread)


def rel_components(name, dev_re, dev_im, ref, rel_re, rel_im, source, report):
    """componentwise relative bars on a complex result"""
    a = mr.check(name + " re", dev_re, [r[0] for r in ref], mr.bar_of([r[0] for r in ref], rel=rel_re), source, report)
    b = mr.check(name + " im", dev_im, [r[1] for r in ref], mr.bar_of([r[1] for r in ref], rel=rel_im), source, report)
    return [a, b]


# ---------------------------------------------------------------------------------------------------------------------
# one function per helper: -> list of rows (math_reference.check)
# ---------------------------------------------------------------------------------------------------------------------
def fexp_small(ctx, report=None):
    (o, _, _, _), _ = run(ctx, "fexp_small", mr.inputs("fexp_small"))
    ref = reference("fexp_small")
    return [mr.check("fexp_small", o, ref, mr.bar_of(ref, nulp=1.5), "mwrt_math.hip.h:144 (2.2e-18 + two rounded FMAs: 1.5 ulp)", report)]


def fexp_tiny(ctx, report=None):
    (o, _, _, _), _ = run(ctx, "fexp_tiny", mr.inputs("fexp_tiny"))
    ref = reference("fexp_tiny")
    return [mr.check("fexp_tiny", o, ref, mr.bar_of(ref, nulp=1.5), "mwrt_math.hip.h:176 (9e-18 + two rounded FMAs: 1.5 ulp)", report)]


def ftanh_half_small(ctx, report=None):
    (o, _, _, _), _ = run(ctx, "ftanh_half_small", mr.inputs("ftanh_half_small"))
    ref = reference("ftanh_half_small")
    return [mr.check("ftanh_half_small", o, ref, mr.bar_of(ref, rel=6e-17, nulp=1.5), "mwrt_math.hip.h:162 (6e-17 + 1.5 ulp)", report)]


def ftanh_half_tiny(ctx, report=None):
    (o, _, _, _), _ = run(ctx, "ftanh_half_tiny", mr.inputs("ftanh_half_tiny"))
    ref = reference("ftanh_half_tiny")
    return [mr.check("ftanh_half_tiny", o, ref, mr.bar_of(ref, rel=3e-21, nulp=1.5), "mwrt_math.hip.h:176 (3e-21 + 1.5 ulp)", report)]


def two_atanh_tail(ctx, report=None):
    """held on 2 atanh(s)/s = 2 + z tail(z): the device tail enters exactly (Decimal), so the error is z |tail - true tail|"""
    z = mr.inputs("two_atanh_tail")[0]
    (o, _, _, _), _ = run(ctx, "two_atanh_tail", (z,))
    ref = reference("two_atanh_tail")
    with mr.decimal.localcontext() as c:
        c.prec = mr.PREC
        full = [2 + mr.dec(zz) * mr.dec(t) for zz, t in zip(z, o)]
        err_ref = [f - r for f, r in zip(full, ref)]
    bar = mr.bar_of(ref, rel=4.6e-18, nulp=1.0)
    err = np.array([abs(float(e)) for e in err_ref])
    mag = np.array([float(r) for r in ref])
    row = dict(points=len(z), worst_err_over_bar=float((err / bar).max()), max_rel=float((err / mag).max()),
               max_ulp=float((err / np.spacing(mag)).max()), bar_rel_max=float((bar / mag).max()), bar_ulp_max=float((bar / np.spacing(mag)).max()),
               bar_from="mwrt_math.hip.h:105 (4.6e-18 on 2 + z tail, + 1 ulp of that)")
    if report is not None:
        report["two_atanh_tail"] = row
    print("two_atanh_tail (on 2 + z tail)  n=%d  max rel %.3e  max ulp %.3f  worst err/bar %.3f" % (
        row["points"], row["max_rel"], row["max_ulp"], row["worst_err_over_bar"]))
    return [row]


def fsqrt(ctx, report=None):
    (o, _, _, _), _ = run(ctx, "fsqrt", mr.inputs("fsqrt"))
    ref = reference("fsqrt")
    return [mr.check("fsqrt", o, ref, mr.bar_of(ref, rel=mr.FSQRT), "mwrt_math.hip.h:276 (2^-45)", report)]


def crecip(ctx, report=None):
    (re, im, _, _), _ = run(ctx, "crecip", mr.inputs("crecip"))
    return rel_components("crecip", re, im, reference("crecip"), 3 * EPS, 3 * EPS, "derived: d eps + reciprocal 1.5 eps (:51) + product eps/2", report)


def cmul_cdiv(ctx, report=None):
    (mre, mim, dre, dim), _ = run(ctx, "cmul_cdiv", mr.inputs("cmul_cdiv"))
    ref = reference("cmul_cdiv")
    rows = []
    for name, dev, k, c, src in (("cmul re", mre, 0, 0, "derived: two products and a sum, eps sum|products|"), ("cmul im", mim, 0, 1, "as cmul re"),
                                 ("cdiv re", dre, 1, 0, "derived: crecip 3 eps + cmul eps, on sum|products|"), ("cdiv im", dim, 1, 1, "as cdiv re")):
        rows.append(mr.check(name, dev, [r[k][c] for r in ref], np.array([float(r[2 + k][c]) for r in ref]), src, report))
    return rows


BAR_CSQRT_A = 1.5 * mr.FSQRT + EPS
BAR_CSQRT_Q = BAR_CSQRT_A + mr.FDIV1 + 0.5 * EPS


def csqrt_principal(ctx, report=None):
    """a (through two fsqrt) is the real part where Re z >= 0 and the imaginary part otherwise; q (one more fdiv1) the other"""
    re, im = mr.inputs("csqrt_principal")
    (ore, oim, _, _), _ = run(ctx, "csqrt_principal", (re, im))
    ref = reference("csqrt_principal")
    pos = re >= 0
    rre, rim = [r[0] for r in ref], [r[1] for r in ref]
    src = "derived from fsqrt 2^-45 twice (:276) and fdiv1 2^-46 (:236): a 4.29e-14, q 5.73e-14"
    return [mr.check("csqrt_principal re", ore, rre, mr.bar_of(rre) + np.where(pos, BAR_CSQRT_A, BAR_CSQRT_Q) * np.abs(np.array(rre, dtype=float)), src, report),
            mr.check("csqrt_principal im", oim, rim, mr.bar_of(rim) + np.where(pos, BAR_CSQRT_Q, BAR_CSQRT_A) * np.abs(np.array(rim, dtype=float)), src, report)]


def _complex_check(name, dre, dim, ref, bar, source, report):
    """|dev - ref| as a complex modulus against an absolute bar per point"""
    with mr.decimal.localcontext() as c:
        c.prec = mr.PREC
        err = np.array([float(mr.c_abs((mr.dec(a) - r[0], mr.dec(b) - r[1]))) for a, b, r in zip(dre, dim, ref)])
        mag = np.array([float(mr.c_abs(r)) for r in ref])
    assert np.all(np.isfinite(dre)) and np.all(np.isfinite(dim)), name
    row = dict(points=len(ref), worst_err_over_bar=float((err / bar).max()), max_rel=float((err / mag).max()),
               max_ulp=float((err / np.spacing(mag)).max()), bar_rel_max=float((bar / mag).max()), bar_from=source)
    if report is not None:
        report[name] = row
    print("%-28s n=%5d  max rel (modulus) %.3e  worst err/bar %.3f  (bar <= %.3e rel; %s)" % (
        name, row["points"], row["max_rel"], row["worst_err_over_bar"], row["bar_rel_max"], source))
    return row


def dcerror_upper(ctx, report=None):
    (re, im, _, _), _ = run(ctx, "dcerror_upper", mr.inputs("dcerror_upper"))
    ref = [r[0] for r in reference("hui")]
    with mr.decimal.localcontext() as c:
        c.prec = mr.PREC
        bar = np.array([5e-15 * float(mr.c_abs(r)) for r in ref])
    return [_complex_check("dcerror_upper", re, im, ref, bar, "mwrt_math.hip.h:311 (5e-15 of |P/Q| on |z| <= 100)", report)]


def hui_w_dw(ctx, report=None):
    (wre, wim, dre, dim), _ = run(ctx, "hui_w_dw", mr.inputs("hui_w_dw"))
    ref = reference("hui")
    src = "derived: 7 complex Horner steps (20 eps S/|p| each polynomial) + crecip"
    return [_complex_check("hui_w_dw w", wre, wim, [r[0] for r in ref], np.array([float(r[2]) for r in ref]), src, report),
            _complex_check("hui_w_dw dw", dre, dim, [r[1] for r in ref], np.array([float(r[3]) for r in ref]), src + ", P' - w Q' term by term", report)]


def planck_inv(x):
    return np.array([float(1 / mr.Fraction(float(v))) for v in x])          # the correctly rounded 1/x


def planck_b_bernoulli(ctx, report=None):
    x = mr.inputs("planck_bernoulli")[0]
    (o, _, _, _), _ = run(ctx, "planck_b", (x, planck_inv(x)))
    ref = reference("planck_b_bernoulli")
    return [mr.check("planck_b Bernoulli", o, ref, mr.bar_of(ref, rel=8e-19, nulp=4.0), "mwrt_math.hip.h:217-221 (8e-19 + 5 FMA roundings: 4 ulp)", report)]


def planck_general_bar(x, ref):
    return np.array([2 * (4e-16 / min(float(v), 1.0) * abs(float(r)) + 1.5 * mr.ulp(r)) for v, r in zip(x, ref)])


def planck_b_general(ctx, report=None):
    x = mr.inputs("planck_general")[0]
    (o, _, _, _), _ = run(ctx, "planck_b", (x, planck_inv(x)))
    ref = reference("planck_b_general")
    return [mr.check("planck_b general", o, ref, planck_general_bar(x, ref), "mwrt_math.hip.h:65-71,233 (2 (4e-16 / min(x, 1) + 1.5 ulp))", report)]


def _lv_bar(ref, waves, per_wave):
    """the bar of each element: 0 at a special case, else the (larger possible) series branch of its wave"""
    bar = np.empty(len(ref))
    for i, r in enumerate(ref):
        hi = waves[i // per_wave][1]
        bar[i] = 0.0 if r[0] in ("negative", "same", "zero") else mr.BAR_LV[hi] * abs(float(r[1]))
    return bar


def layer_value(ctx, report=None, names=("layer_value_zf1", "layer_value_zf0", "layer_value4")):
    x1, x0, live = mr.inputs("layer")
    rows = []
    for name in names:
        ref = layer_reference(name != "layer_value_zf0")
        per = 4 if name == "layer_value4" else 1
        (o, _, _, _), _ = run(ctx, name, (x1, x0, live))
        idx = np.flatnonzero(live != 0)             # a lane that is not live holds no layer: its result is unused (whole quads)
        bar = _lv_bar(ref, layer_waves(per), mr.WAVE * per)
        rows.append(mr.check(name, o[idx], [ref[i][1] for i in idx], bar[idx],
                             "derived (mwrt_layer.hip.h): small 6.3e-16, mid 2.33e-14, any 2.92e-14 by the wave's branch; special cases exact", report))
    return rows


def tl_bars(x1, x0, ref):
    """(value bar, partial bar): absolute; the partials' is one number per point for both (relative to max(|d1|, |d0|))"""
    bv, bp = np.zeros(len(ref)), np.zeros(len(ref))
    for i, (br, L, d1, d0) in enumerate(ref):
        if br in ("negative", "same", "zero"):
            continue
        L, d1, d0 = float(L), float(d1), float(d0)
        if br == "small" and abs(float(mr.exact_abs_s(x1[i], x0[i])) / mr.LOGMEAN_SMALL_S - 1) > mr.SWITCH_SLACK:
            bv[i] = mr.BAR_TL["small"] * abs(L)
            bp[i] = mr.BAR_TL_PARTIAL_SMALL * max(abs(d1), abs(d0))
        else:
            iln = abs(L / (x1[i] - x0[i]))
            relL = mr.BAR_TL["any"]
            bv[i] = relL * abs(L)
            b1 = (L / x1[i] * (relL + 1.5 * EPS) + EPS) * iln + 2.5 * EPS * abs(d1)
            b0 = (L / x0[i] * (relL + 1.5 * EPS) + EPS) * iln + 2.5 * EPS * abs(d0)
            bp[i] = max(b1, b0)
            if br == "small":                                               # at the switch either branch may be taken
                bp[i] = max(bp[i], mr.BAR_TL_PARTIAL_SMALL * max(abs(d1), abs(d0)))
    return bv, bp


def layer_value_tl(ctx, report=None):
    x1, x0, live = mr.inputs("layer")
    rows = []
    for name in ("layer_value_tl_zf1", "layer_value_tl_zf0"):
        ref = layer_reference(name.endswith("zf1"))
        (o, d1, d0, _), _ = run(ctx, name, (x1, x0, live))
        bv, bp = tl_bars(x1, x0, ref)
        src = "derived (mwrt_tl_dev.hip.h): small 3 eps / partials 4 eps; else flog + two fdiv 2.0e-15, partials term by term"
        rows.append(mr.check(name + " value", o, [r[1] for r in ref], bv, src, report))
        rows.append(mr.check(name + " d/dx1", d1, [r[2] for r in ref], bp, src, report))
        rows.append(mr.check(name + " d/dx0", d0, [r[3] for r in ref], bp, src, report))
    return rows


CHECKS = {"fexp_small": fexp_small, "fexp_tiny": fexp_tiny, "ftanh_half_small": ftanh_half_small, "ftanh_half_tiny": ftanh_half_tiny,
          "two_atanh_tail": two_atanh_tail, "fsqrt": fsqrt, "crecip": crecip, "cmul_cdiv": cmul_cdiv, "csqrt_principal": csqrt_principal,
          "dcerror_upper": dcerror_upper, "hui_w_dw": hui_w_dw, "planck_b_bernoulli": planck_b_bernoulli,
          "planck_b_general": planck_b_general, "layer_value": layer_value, "layer_value_tl": layer_value_tl}
