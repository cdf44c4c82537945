"""TEST INFRASTRUCTURE ONLY -- an exact derivative reference for the device K-matrix.

The clear-sky, plane-parallel path of ``oracle/lbl_oracle.py`` restated in torch float64 on the CPU, statement by
statement (vectorised over frequencies and levels), so that torch autograd yields derivatives of the oracle's own
formulas that are exact up to rounding.  ``tests/test_tl_oracle.py`` pins its values to ``lbl_oracle`` and its
derivatives to central differences of ``lbl_oracle``; ``tests/test_jacobian_device_edges.py`` checks
``mwrt_absorption_tl_batch_device`` and ``mwrt_tb_jacobian_batch_device`` against it row by row.

Nothing here touches the native library or a GPU: the reference shares neither code nor a device with the kernels it
checks.  Where the oracle's formulas branch or are not differentiable, the derivative follows the device's documented
tangent conventions; each is written down where it is applied:

* a dry level (rho <= 0): the value is zeroed as in pyrtlib and the tangent is kept -- the right-sided derivative;
* ``max(o2abs, 0)``: zero slope where it clamps;
* the layer rule's ``|x1 - x0| < 1e-9`` branch: partials (1, 0); a zero end value: partials (0.5, 0.5);
* the speed-dependent switch and the 750-GHz cutoff: the derivative of the branch that is taken.

Every ``torch.where`` whose untaken branch could be NaN or inf feeds that branch a safe stand-in first ("double
where"): autograd multiplies the untaken branch's gradient by zero, and 0 * inf would turn the gradient NaN silently.

Partial derivatives are the device ABI's: T at fixed e, e at fixed T, layer thickness (``z = z0 + cumsum(dz)``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

RWATVAP = 461.5
TAUMAX = 125.0
F64 = torch.float64


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=F64)


def vapor(tk, rh):
    """lbl_oracle.vapor: Goff-Gratch over water.  tk [K], rh [fraction] -> e [hPa], rho [g m-3]."""
    rvap = RWATVAP * 1e-05
    y = 373.16 / tk
    es = (-7.90298 * (y - 1.0) + 5.02808 * torch.log10(y)
          - 1.3816e-07 * (10.0 ** (11.344 * (1.0 - (1.0 / y))) - 1.0)
          + 0.0081328 * (10.0 ** (-3.49149 * (y - 1.0)) - 1.0) + math.log10(1013.246))
    es = 10.0 ** es
    e = rh * es
    rho = e / (rvap * tk)
    return e, rho


_HUI_A = [122.607931777104326, 214.382388694706425, 181.928533092181549, 93.155580458138441, 30.180142196210589,
          5.912626209773153, 0.564189583562615]
_HUI_B = [122.607931773875350, 352.730625110963558, 457.334478783897737, 348.703917719495792, 170.354001821091472,
          53.992906912940207, 10.479857114260399]


def dcerror(x, y):
    """lbl_oracle.dcerror: Hui, Armstrong & Wray's rational for w(z), z = x + iy, both half-planes."""
    a, b = _HUI_A, _HUI_B
    zh = torch.complex(torch.abs(y), -x)
    asum = (((((a[6] * zh + a[5]) * zh + a[4]) * zh + a[3]) * zh + a[2]) * zh + a[1]) * zh + a[0]
    bsum = ((((((zh + b[6]) * zh + b[5]) * zh + b[4]) * zh + b[3]) * zh + b[2]) * zh + b[1]) * zh + b[0]
    w = asum / bsum
    neg = y < 0
    if bool(neg.any()):
        # double where: exp(-z^2) overflows for large |x| where the lower half-plane form is not taken
        z = torch.complex(torch.where(neg, x, torch.zeros_like(x)), torch.where(neg, y, torch.zeros_like(y)))
        w2 = 2.0 * torch.exp(-z ** 2) - torch.conj(w)
        w = torch.where(neg, w2, w)
    return w


def h2o_absorption(m, pdrykpa, vx, ekpa, frq):
    """lbl_oracle.h2o_absorption.  Level arrays [nlev], frq [nf, 1] -> (npp, ncpp) [nf][nlev]."""
    db2np = math.log(10.0) * 0.1
    rvap = (0.01 * 8.314510) / 18.01528
    factor = 0.182 * frq
    t = 300.0 / vx
    p = (pdrykpa + ekpa) * 10.0
    rho = ekpa * 10.0 / (rvap * t)
    f = frq
    pvap = (rho * t) / m.h2o_pvap_div
    pda = p - pvap
    den = m.h2o_den_coef * rho
    ti = m.h2o_reftcon / t
    con = (m.h2o_cf * pda * ti ** m.h2o_xcf + m.h2o_cs * pvap * ti ** m.h2o_xcs) * pvap * f * f
    ti = m.h2o_reftline / t
    tiln = torch.log(ti)
    if m.h2o_shift_mode == 0:
        ti2 = ti ** 2.5
    else:
        ti2 = torch.exp(2.5 * tiln)
    L = m.h2o
    summ = torch.zeros(f.shape[0], t.shape[0], dtype=F64)
    for i in range(len(L["fl"])):
        width0 = L["w0"][i] * pda * ti ** L["x"][i] + L["w0s"][i] * pvap * ti ** L["xs"][i]
        if L["w2"][i] > 0:
            width2 = L["w2"][i] * pda * ti ** L["xw2"][i] + L["w2s"][i] * pvap * ti ** L["xw2s"][i]
        else:
            width2 = torch.zeros_like(t)
        delta2 = L["d2"][i] * pda + L["d2s"][i] * pvap
        if m.h2o_shift_mode == 0:
            shift = torch.zeros_like(t)
        else:
            shiftf = L["sh"][i] * pda * (1.0 - L["aair"][i] * tiln) * ti ** L["xh"][i]
            shifts = L["shs"][i] * pvap * (1.0 - L["aself"][i] * tiln) * ti ** L["xhs"][i]
            shift = shiftf + shifts
        wsq = width0 ** 2
        s = L["s1"][i] * ti2 * torch.exp(L["b2"][i] * (1.0 - ti))
        df = [f - L["fl"][i] - shift, f + L["fl"][i] + shift]
        base = width0 / (562500.0 + wsq)
        res = torch.zeros_like(summ)
        for j in range(2):
            # the 750-GHz cutoff: the branch that is taken (the cut branch is a constant 0, no NaN to guard)
            lor = torch.where(torch.abs(df[j]) < 750.0, width0 / (df[j] ** 2 + wsq) - base, torch.zeros_like(summ))
            if j == 0 and L["w2"][i] > 0:
                # the speed-dependent switch: the branch that is taken.  Double where: outside the switch the SD
                # expression is evaluated at a harmless stand-in (A = 1, B = 1) so its zero gradient stays finite
                use_sd = (width2 > 0) & (torch.abs(df[j]) < 10.0 * width0)
                if bool(use_sd.any()):
                    one = torch.ones_like(summ)
                    w0s = torch.where(use_sd, width0.expand_as(summ), one)
                    w2s = torch.where(use_sd, width2.expand_as(summ), one)
                    d2s = torch.where(use_sd, delta2.expand_as(summ), 0.0 * one)
                    dfs = torch.where(use_sd, df[j], 0.0 * one)
                    B = torch.complex(w2s, -d2s)
                    xc = torch.complex(w0s - 1.5 * w2s, dfs + 1.5 * d2s) / B
                    xrt = torch.sqrt(xc)
                    pxw = 1.77245385090551603 * xrt * dcerror(-xrt.imag, xrt.real)
                    sd = 2.0 * (1.0 - pxw) / B
                    lor = torch.where(use_sd, sd.real - base, lor)
            res = res + lor
        summ = summ + s * res * (f / L["fl"][i]) ** 2
    npp = (3.183e-05 * den * summ / db2np) / factor
    ncpp = (con / db2np) / factor
    # a dry level: pyrtlib zeroes the value; the tangent is kept (the right-sided derivative at e = 0).
    # a - a.detach() is 0 in value and carries a's gradient
    zero = rho <= 0.0
    npp = torch.where(zero, npp - npp.detach(), npp)
    ncpp = torch.where(zero, ncpp - ncpp.detach(), ncpp)
    return npp, ncpp


def n2_absorption(m, t, p, f):
    """lbl_oracle.n2_absorption (Np/km)."""
    th = 300.0 / t
    fdepen = 0.5 + 0.5 / (1.0 + (f / 450.0) ** 2) if m.n2_fdep else 1.0
    bf = m.n2_l * fdepen * p * p * f * f * th ** m.n2_m
    return m.n2_n * bf


def o2_absorption(m, pdrykpa, vx, ekpa, frq):
    """lbl_oracle.o2_absorption.  Level arrays [nlev], frq [nf, 1] -> (npp, ncpp) [nf][nlev]."""
    db2np = math.log(10.0) * 0.1
    rvap = (0.01 * 8.314510) / 18.01528
    factor = 0.182 * frq
    temp = 300.0 / vx
    pres = (pdrykpa + ekpa) * 10.0
    vapden = (ekpa * 10.0) / (rvap * temp)
    freq = frq
    th = 300.0 / temp
    th1 = th - 1.0
    b = th ** m.o2_x
    preswv = vapden * temp / m.o2_pvap_div
    presda = pres - preswv
    den = 0.001 * (presda * b + m.o2_wv_factor * preswv * th)
    dens = 0.001 * (presda + m.o2_wv_factor * preswv) * th
    dfnr = m.o2_wb300 * den
    pe2 = den * den
    nonres = m.o2_nonres * freq * freq * dfnr / (th * (freq * freq + dfnr * dfnr))
    summ = nonres.clone()
    L = m.o2
    for k in range(len(L["f"])):
        if m.o2_mix_mode == 0:
            df = L["w300"][k] * (dens if (k == 0 and m.o2_line1_dens) else den)
            y = 0.001 * pres * b * (L["y0"][k] + L["y1"][k] * th1)
            strr = L["s300"][k] * torch.exp(-L["be"][k] * th1)
            sf1 = (df + (freq - L["f"][k]) * y) / ((freq - L["f"][k]) ** 2 + df * df)
            sf2 = (df - (freq + L["f"][k]) * y) / ((freq + L["f"][k]) ** 2 + df * df)
        else:
            y = den * (L["y0"][k] + L["y1"][k] * th1)
            dnu = pe2 * (L["dnu0"][k] + L["dnu1"][k] * th1)
            gfac = 1.0 + pe2 * (L["g0"][k] + L["g1"][k] * th1)
            df = L["w300"][k] * den
            strr = L["s300"][k] * torch.exp(-L["be"][k] * th1)
            del1 = freq - L["f"][k] - dnu
            del2 = freq + L["f"][k] + dnu
            d1 = del1 * del1 + df * df
            d2 = del2 * del2 + df * df
            sf1 = (df * gfac + del1 * y) / d1
            sf2 = (df * gfac - del2 * y) / d2
        summ = summ + strr * (sf1 + sf2) * (freq / L["f"][k]) ** 2
    o2abs = m.o2_coef * summ * presda * th ** 3
    # max(o2abs, 0): zero slope where it clamps (the device's !(o2 > 0) -> 0)
    o2abs = torch.where(o2abs > 0.0, o2abs, torch.zeros_like(o2abs))
    ncpp = m.o2_coef * nonres * presda * th ** 3
    npp = (o2abs / db2np) / factor - (ncpp / db2np) / factor
    ncpp = (ncpp / db2np) / factor
    if m.n2_ptot:
        ncpp = ncpp + (n2_absorption(m, temp, pres, freq) / db2np) / factor
    return npp, ncpp


def clearsky_absorption(m, p, tk, e, frq):
    """lbl_oracle.clearsky_absorption for every frequency at once: p, tk, e [nlev]; frq [nf] -> awet, adry [nf][nlev]."""
    frq = _t(frq).reshape(-1, 1)
    factor = 0.182 * frq
    db2np = math.log(10.0) * 0.1
    v = 300.0 / tk
    ekpa = e / 10.0
    pdrykpa = p / 10.0 - ekpa
    npp, ncpp = h2o_absorption(m, pdrykpa, v, ekpa, frq)
    awet = (factor * (npp + ncpp)) * db2np
    npp, ncpp = o2_absorption(m, pdrykpa, v, ekpa, frq)
    ao2 = (factor * (npp + ncpp)) * db2np
    an2 = 0.0 if m.n2_ptot else n2_absorption(m, tk, pdrykpa * 10.0, frq)
    adry = ao2 + an2
    return awet, adry


class _LogMean(torch.autograd.Function):
    """(x1 - x0) / log(x1 / x0), the value as the oracle computes it, with partials that stay accurate for close levels.

    Float64 autograd of the quotient forms dL/dx1 = (1 - L/x1) / ln, where both the numerator and ln cancel for close
    values: it loses ~eps / s^2 relative (s = (x1 - x0) / (x1 + x0); 2e-8 at s = 1e-4, a 2-m layer).  Here, with
    u = (x1 - x0) / x0 (x1 - x0 is exact for close values) and phi(u) = u / log1p(u), so that L = x0 phi(u):
        dL/dx1 = phi'(u) = N(u) / log1p(u)^2,   dL/dx0 = phi(u) - (1 + u) phi'(u),
        N(u) = log1p(u) - u / (1 + u) = sum_{k >= 2} (-1)^k (k - 1) / k u^k,
    N summed as its Taylor series (63 terms: the remainder is below 1e-17 of N), used where |u| < 0.5; elsewhere the
    quotient's own partials, which are well conditioned there."""

    @staticmethod
    def forward(ctx, x1, x0):
        ln = torch.log(x1 / x0)
        L = (x1 - x0) / ln
        u = (x1 - x0) / x0
        close = torch.abs(u) < 0.5
        uc = torch.where(close, u, torch.full_like(u, 0.25))   # (a harmless stand-in where the series is not used)
        ser = torch.zeros_like(u)
        for k in range(64, 1, -1):                      # Horner: N = u^2 sum_{k>=2} c_k u^(k-2)
            ser = ser * uc + (-1) ** k * (k - 1) / k
        l1c = torch.log1p(uc)
        dphi = uc * uc * ser / (l1c * l1c)
        # far apart (one end may be ~1e-17 of the other, where u rounds to -1): the quotient's own partials are accurate
        d1 = torch.where(close, dphi, (1.0 - L / x1) / ln)
        d0 = torch.where(close, uc / l1c - (1.0 + uc) * dphi, (L / x0 - 1.0) / ln)
        ctx.save_for_backward(d1, d0)
        return L

    @staticmethod
    def backward(ctx, g):
        d1, d0 = ctx.saved_tensors
        return g * d1, g * d0


def exponential_integration(x, ds):
    """lbl_oracle.exponential_integration (zeroflg True) for every row at once: x, ds [..., nlev] -> xds [..., nlev]
    (xds[..., 0] = 0), in the oracle's branch order.  The two special branches' derivatives are those of the values they
    return: |x1 - x0| < 1e-9 -> x1, partials (1, 0); a zero end -> (x1 + x0) / 2, partials (0.5, 0.5).  The general
    branch's partials come from _LogMean (well conditioned for close values)."""
    if bool((x < 0.0).any()):
        raise ValueError("Error encountered in exponential_integration")
    x1, x0 = x[..., 1:], x[..., :-1]
    small = torch.abs(x1 - x0) < 1e-09
    zero = (x0 == 0.0) | (x1 == 0.0)
    general = ~small & ~zero
    # double where: log(x1 / x0) is inf / NaN at a zero end and 0 for equal values; the general branch sees 2 and 1 there
    g1 = torch.where(general, x1, torch.full_like(x1, 2.0))
    g0 = torch.where(general, x0, torch.ones_like(x0))
    xlayer = torch.where(small, x1, torch.where(zero, (x1 + x0) * 0.5, _LogMean.apply(g1, g0)))
    xds = xlayer * ds[..., 1:]
    return torch.cat([torch.zeros_like(xds[..., :1]), xds], dim=-1)


def planck_down(m, frq, tk, taulay):
    """lbl_oracle.planck_down -> boftotl, for every row at once: frq [nf, 1, 1] (broadcast against taulay
    [nf, nang, nlev]), tk [nlev].  The recursion is written with cumulative sums: tauprof_i = sum_{k <= i} taulay_k,
    boftatm_n = sum_i boftlay_i exp(-tauprof_{i-1}) (1 - exp(-taulay_i))."""
    hvk = (frq * 1e9) * m.planck_h / m.boltzmann_k
    boft = 1.0 / (torch.exp(hvk / tk) - 1.0)
    lay = taulay[..., 1:]
    E = torch.exp(-lay)
    boftlay = (boft[..., :-1] + boft[..., 1:] * E) / (1.0 + E)
    tauprof = torch.cumsum(taulay, dim=-1)
    batmlay = boftlay * torch.exp(-tauprof[..., :-1]) * (1.0 - E)
    boftatm = torch.sum(batmlay, dim=-1)
    tautot = tauprof[..., -1]
    boftbg = 1.0 / (torch.exp(hvk[..., 0] / m.t_cosmic) - 1.0)
    bakgrnd = boftbg * torch.exp(-tautot)
    # tauprof < TAUMAX: the cosmic term is added; opaque paths leave it out (both branches are finite)
    boftotl = torch.where(tautot < TAUMAX, bakgrnd + boftatm, boftatm)
    return boftotl, hvk[..., 0], tautot


def bright(hvk, boft):
    return hvk / torch.log(1.0 + (1.0 / boft))


def _amass(angles):
    return 1 / torch.sin(_t(angles) * math.pi / 180)


def tb_from_ds(m, dsz, p, tk, e, frq, angles):
    """TBs [nang][nf] from zenith layer thicknesses dsz [nlev] (dsz[0] = 0: the ground has no layer below it)."""
    awet, adry = clearsky_absorption(m, p, tk, e, frq)                  # [nf][nlev]
    return tb_from_absorption(m, awet, adry, dsz, tk, frq, angles)


def tb_from_absorption(m, awet, adry, dsz, tk, frq, angles):
    """The RTE half of tb_cloud_rte: awet, adry [nf][nlev] -> TBs [nang][nf]."""
    ds = dsz.reshape(1, -1) * _amass(angles).reshape(-1, 1)             # [nang][nlev], as np.diff(z) * amass
    pw = exponential_integration(awet[:, None, :], ds)                  # [nf][nang][nlev]
    pd = exponential_integration(adry[:, None, :], ds)
    taulay = pw + pd
    boftotl, hvk, _ = planck_down(m, _t(frq).reshape(-1, 1, 1), tk, taulay)
    return bright(hvk, boftotl).T                                       # [nang][nf]


def tb_z(m, z, p, tk, e, frq, angles):
    """tb_cloud_rte's tbtotal [nang][nf] from heights z [nlev], as the oracle forms its layers (z - z[0], then diff)."""
    zz = z - z[0]
    dsz = torch.cat([torch.zeros_like(zz[:1]), zz[1:] - zz[:-1]])
    return tb_from_ds(m, dsz, p, tk, e, frq, angles)


def tb_dz(m, dz, p, tk, e, frq, angles):
    """TBs [nang][nf] as a function of layer thicknesses dz [nlev] (dz[0] unused: z = z0 + cumsum(dz)), p, T and e."""
    dsz = torch.cat([torch.zeros_like(dz[:1]), dz[1:]])
    return tb_from_ds(m, dsz, p, tk, e, frq, angles)


def tb_rh(m, z, p, t, rh, frq, angles):
    """The (z, p, t, rh) form of the operator autodiff.brightness_temperature differentiates: TBs [nang][nf]."""
    e, _ = vapor(t, rh)
    return tb_z(m, z, p, t, e, frq, angles)


# ---- Jacobians in the device ABI's layout ------------------------------------------------------------------------
def _rows(y, xs):
    """Gradients of every element of y (any shape) with respect to each of xs: [*y.shape, len(x)] per x."""
    flat = y.reshape(-1)
    out = [torch.zeros(flat.numel(), x.numel(), dtype=F64) for x in xs]
    for k in range(flat.numel()):
        g = torch.autograd.grad(flat[k], xs, retain_graph=True, allow_unused=True)
        for o, gi in zip(out, g):
            if gi is not None:
                o[k] = gi.reshape(-1)
    return [o.reshape(*y.shape, -1) for o in out]


def absorption_tl(m, p, tk, e, frq):
    """awet, adry [nf][nlev] and their exact partials d/dT at fixed e, d/de at fixed T (absorption is local to a level,
    so the gradient of a row's sum is the row of diagonal partials).  Inputs are float64 arrays or tensors [nlev]."""
    p = _t(p)
    tk = _t(tk).clone().requires_grad_(True)
    e = _t(e).clone().requires_grad_(True)
    aw, ad = clearsky_absorption(m, p, tk, e, frq)
    out = {"awet": aw.detach(), "adry": ad.detach()}
    for name, a in (("awet", aw), ("adry", ad)):
        dt = torch.zeros_like(a.detach())
        de = torch.zeros_like(a.detach())
        for j in range(a.shape[0]):
            gt, ge = torch.autograd.grad(a[j].sum(), (tk, e), retain_graph=True)
            dt[j], de[j] = gt, ge
        out[f"d{name}_dt"], out[f"d{name}_de"] = dt, de
    return out


def k_matrix(m, z, p, tk, e, frq, angles):
    """The device K-matrix of one profile: tb [nang][nf] and dtb_dt, dtb_de, dtb_ddz [nang][nf][nlev] (T at fixed e,
    e at fixed T, thickness of the layer below each level; level 0 has none).

    Autograd through two stages joined by the chain rule: the exact absorption partials (local per level) and the
    gradients of each TB with respect to the absorption rows, T (the Planck terms) and the layer thicknesses."""
    with torch.enable_grad():                  # (also when called inside an autograd Function's forward)
        return _k_matrix(m, z, p, tk, e, frq, angles)


def _k_matrix(m, z, p, tk, e, frq, angles):
    z, p, tk, e = (_t(x) for x in (z, p, tk, e))
    ab = absorption_tl(m, p, tk, e, frq)
    aw = ab["awet"].clone().requires_grad_(True)
    ad = ab["adry"].clone().requires_grad_(True)
    tq = tk.clone().requires_grad_(True)
    zz = z - z[0]
    dsz = torch.cat([torch.zeros_like(zz[:1]), zz[1:] - zz[:-1]]).requires_grad_(True)
    tb = tb_from_absorption(m, aw, ad, dsz, tq, frq, angles)                  # [nang][nf]
    nang, nf = tb.shape
    nlev = z.shape[0]
    jf = torch.arange(nf)
    g_aw, g_ad, g_t, g_dz = _rows(tb, (aw, ad, tq, dsz))                      # [nang][nf][nf*nlev or nlev]
    g_aw = g_aw.reshape(nang, nf, nf, nlev)[:, jf, jf, :]                    # a TB row depends on its own frequency only
    g_ad = g_ad.reshape(nang, nf, nf, nlev)[:, jf, jf, :]
    dt = g_aw * ab["dawet_dt"] + g_ad * ab["dadry_dt"] + g_t
    de = g_aw * ab["dawet_de"] + g_ad * ab["dadry_de"]
    return {"tb": tb.detach(), "dtb_dt": dt, "dtb_de": de, "dtb_ddz": g_dz}


def k_matrix_rh(m, z, p, t, rh, frq, angles):
    """k_matrix from the (z, p, t, rh) inputs the device entry takes (e = rh * es(T) as RTEquation.vapor)."""
    e, _ = vapor(_t(t), _t(rh))
    return k_matrix(m, z, p, t, e.detach(), frq, angles)


def direct_gradients(m, z, p, t, rh, frq, angles, weights=None):
    """Autograd of sum(weights * TB) with respect to z, t and rh (the variables autodiff.brightness_temperature exposes).
    weights [nang][nf] (default: ones).  -> {"z", "t", "rh"} [nlev] each."""
    xs = [_t(x).clone().requires_grad_(True) for x in (z, t, rh)]
    tb = tb_rh(m, xs[0], _t(p), xs[1], xs[2], frq, angles)
    w = torch.ones_like(tb) if weights is None else _t(weights)
    gz, gt, grh = torch.autograd.grad((w * tb).sum(), xs)
    return {"z": gz, "t": gt, "rh": grh}


def branch_margins(m, p, tk, e, frq):
    """For each (frequency, level): the smallest relative distance of an absorption branch predicate from its threshold
    (the 750-GHz cutoffs and the speed-dependent switch).  A kernel may take the other branch only where this
    is at rounding level.  -> [nf][nlev] numpy."""
    p, tk, e = (_t(x) for x in (p, tk, e))
    with torch.no_grad():
        frq = _t(frq).reshape(-1, 1)
        ekpa = e / 10.0
        pdrykpa = p / 10.0 - ekpa
        t = tk
        pvap = (ekpa * 10.0 / ((0.01 * 8.314510) / 18.01528 * t) * t) / m.h2o_pvap_div
        pda = (pdrykpa + ekpa) * 10.0 - pvap
        ti = m.h2o_reftline / t
        tiln = torch.log(ti)
        L = m.h2o
        margin = torch.full((frq.shape[0], t.shape[0]), math.inf, dtype=F64)
        for i in range(len(L["fl"])):
            shift = 0.0
            if m.h2o_shift_mode != 0:
                shift = (L["sh"][i] * pda * (1.0 - L["aair"][i] * tiln) * ti ** L["xh"][i]
                         + L["shs"][i] * pvap * (1.0 - L["aself"][i] * tiln) * ti ** L["xhs"][i])
            for df in (frq - L["fl"][i] - shift, frq + L["fl"][i] + shift):
                margin = torch.minimum(margin, torch.abs(torch.abs(df) - 750.0) / 750.0)
            if L["w2"][i] > 0:
                w0 = L["w0"][i] * pda * ti ** L["x"][i] + L["w0s"][i] * pvap * ti ** L["xs"][i]
                lim = 10.0 * torch.abs(w0)
                margin = torch.minimum(margin, torch.abs(torch.abs(frq - L["fl"][i] - shift) - lim) / lim)
    return margin.numpy()
