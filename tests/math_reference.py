"""High-precision references, input sets and error bars for the device arithmetic helpers (csrc/mwrt_math.hip.h,
csrc/mwrt_layer.hip.h, csrc/mwrt_tl_dev.hip.h) as mwrt_selftest_helpers runs them.  Standard library only (``decimal`` at
PREC = 50 digits, ``fractions`` where exact) plus numpy for the arrays: tests/test_math_helpers.py (GPU),
tests/test_math_reference.py (CPU, checks this module against itself) and tools/math_helper_errors.py share it.

Errors are exact: the device double converted to ``Decimal``, minus the reference.  A bar is an ABSOLUTE bound per point,
``rel * |ref| + nulp * ulp(ref)`` (``ulp(ref)`` = the spacing of doubles at ``|ref|``), or a per-point bound computed from the
reference's own magnitudes; ``check`` reports the largest error/bar ratio together with the largest relative and ulp errors.

DOMAINS (the call sites they were read from; the input sets below fill them and add both ends, +-0 where defined, and
values within 4 ulp either side of every internal switch)
  fexp_small        |x| <= 1/8: -tl under ``wave_all(fabs(tl) <= EXP_SMALL_X)`` (mwrt_fused.hip.h:525, :507, :537; mwrt_tau.hip.h:410)
  fexp_tiny, ftanh_half_tiny   |x| <= 1/64 (mwrt_tau.hip.h:420-421, behind the EXP_TINY_X vote)
  ftanh_half_small  0 <= x <= 1/8 (mwrt_fused.hip.h:508/538, mwrt_tau.hip.h:411, mwrt_tl_rte.hip.h:326 ``tau <= EXP_SMALL_X``);
                    the function is odd and the negative half is run as well
  two_atanh_tail    0 <= z <= 0.1716^2 (flog, mwrt_math.hip.h:137; log_mean_any, mwrt_layer.hip.h:65)
  planck_b          x = h f / (k T), f 1..1000 GHz, T 100..350 K: 1.4e-4 .. 0.48, and on to 5 (mwrt_fused.hip.h:381,
                    mwrt_tau.hip.h:394/407, mwrt_tl_rte.hip.h:266); inv_x the correctly rounded 1/x
  fsqrt             T/M with T 100..350 K, M 16..50 (mwrt_absorption.hip.h:869); 0.2166 wc^2 + 0.6931 bd^2 with widths of
                    1e-8 .. 10 GHz (:878); |z|^2 and (|z| + |Re z|)/2 of csqrt_principal: 1e-16 .. 1e8 in all
  csqrt_principal   xc = (w0 - 1.5 w2 + i (d1 + 1.5 delta2)) / (w2 - i delta2), |d1| < 10 w0 (mwrt_absorption.hip.h:486-497,
                    :544-545): with w2 a fraction of w0 and |delta2| << w2, Re xc > 0 and |xc| ~ (w0 / w2) (1 .. 10), a few to
                    a few thousand; filled as |xc| 1e-4 .. 1e4, a third of it with Re > 0.  The helper serves either sign of
                    Re z, so the disc |z| <= 1e4 (|sqrt z| <= 100) is filled on both sides of the cut as well
  dcerror_upper, hui_w_dw   zh = the principal root above: Re zh >= 0, |zh| <= 100 (mwrt_math.hip.h:311)
  crecip, cmul, cdiv   components 1e-6 .. 1e4 of either sign (w2 - i delta2, mwrt_absorption.hip.h:495; the Debye terms, :833-846)
  layer_value*      absorption coefficients of adjacent levels, 1e-12 .. 1e2 Np/km, ratios up to 1e6, with the special cases
                    (mwrt_fused.hip.h:276/316, mwrt_tau.hip.h:138, mwrt_tl_rte.hip.h:207/275)
  div_small         0 <= n < 65536, 1 <= d <= 1024 (mwrt_plan.h:21; mwrt_fused.hip.h:456-480)

BARS.  eps = 2^-52 (one ulp, relative, at most).  Those the source states are used as stated (mwrt_math.hip.h):
  fexp_small, fexp_tiny   1.5 ulp (:144, :176: truncation 2.2e-18 / 9e-18 and the two rounded FMAs at the end)
  ftanh_half_small / tiny   6e-17 / 3e-21 relative + 1.5 ulp (:162, :176)
  two_atanh_tail    4.6e-18 relative on 2 atanh(s)/s = 2 + z tail(z), + 1 ulp of that (:105)
  fsqrt             2^-45 (:276);   fdiv1 2^-46 = 1.42e-14 (:236);   fdiv-grade reciprocal 1.5 eps (:51)
  dcerror_upper     5e-15 relative to |P/Q|, against the exact rational (:311)
  planck_b          Bernoulli branch 8e-19 + 4 ulp (:217-221); general branch 2 (4e-16 / min(x, 1) + 1.5 ulp) (:65-71, :233)
Derived (a correctly rounded operation costs eps/2):
  crecip            d = fma(re, re, im im): eps; the Newton reciprocal: 1.5 eps; the product: eps/2 -> 3 eps per component
  cmul              each component is two products and a sum: eps (|a.re b.re| + |a.im b.im|) resp. eps (|a.re b.im| + |a.im b.re|)
  cdiv              cmul(a, crecip(b)): (3 + 1) eps (|a.re c.re| + |a.im c.im|), c = 1/b exact (likewise the imaginary part)
  csqrt_principal   r = fsqrt(|z|^2): the argument carries eps, halved by the root, + 2^-45.  a = fsqrt((r + |Re z|)/2): the
                    argument carries r's error + eps/2, halved, + 2^-45 -> a: 1.5 * 2^-45 + eps = 4.29e-14.
                    q = fdiv1(Im z, 2a): a's error + 2^-46 + eps/2 -> 5.73e-14.  No cancellation: r + |Re z| adds positives.
  hui_w_dw          Horner at a complex point, n = 7 steps of one complex product (<= 2 sqrt2 u relative, u = eps/2) and one
                    real add: |err P| <= 20 eps S_P with S_P = sum |a_k| |zh|^k, likewise Q (the usual gamma_2n bound with the
                    complex constant); w = P crecip(Q): + 5 eps.  bar_w = |w| (20 eps (S_P/|P| + S_Q/|Q|) + 5 eps).
                    dw = (P' - w Q') / Q: bar = (20 eps S_P' + |w| 20 eps S_Q' + |Q'| bar_w + 2 eps (|P'| + |w Q'|)) / |Q|
                    + 5 eps |dw|, S_P' = sum k |a_k| |zh|^(k-1): the cancellation in P' - w Q' is paid for where it happens.
  layer_value, layer_value4 (mwrt_layer.hip.h), relative to the log-mean, by the series branch the WAVE takes:
    s = fdiv1(d, sm), d and sm rounded: REL_S = 2^-46 + 1.5 eps.  q(z) = s/atanh(s), z = s^2, has kappa = |z q'/q|.
    small  |s| <= 0.1715: kappa <= 0.0101 -> 2 kappa REL_S = 2.9e-16, + the fit 1.1e-18 + 1.5 eps (final FMA, sm, product) = 6.3e-16
    mid    |s| <= 0.6: kappa <= 0.1763 -> 5.1e-15; fdiv1(pn, qd) 2^-46; pn and qd alternate in sign with sum|c z^k| / |p| <= 7.7
           and 6.0 -> 14 eps; the fit 7.7e-17; + 2 eps = 2.33e-14
    any    sp = fdiv1(..): REL_S; two_atanh_tail 4.6e-18; |e ln2 + ln m| >= |ln m| (|ln m| <= ln2 / 2), so ln carries REL_S + eps;
           fdiv1(d, ln): 2^-46 + eps/2; d: eps/2 -> 2 * 2^-46 + 3.5 eps = 2.92e-14
    A lane whose exact |s| lies within 1e-12 relative of a switch may be voted either way (the device compares its own
    rounded s): its wave is held to the larger of the two bars.  The special cases are exact (bar 0).
  layer_value_tl (mwrt_tl_dev.hip.h), branch per LANE, s from fdiv:
    small  10-term Taylor series (next term 1e-19), s to 2.5 eps with kappa 0.01, q + 1, sm/2 q: 3 eps;
           partials q/2 +- 2 s q' x/sm ~ 1/2: 4 eps of max(|d1|, |d0|)
    else   ln = flog(fdiv(x1, x0)): the ratio's 1.5 eps is 1.5 eps / |ln| <= 4.3 eps of ln (|ln| >= 2 atanh 0.1715), flog
           itself 5e-16 (the bar tests/test_gpu_parity.py holds it to); iln, d, product: 2.5 eps -> 6.8 eps + 5e-16 = 2.0e-15.
           d1 = (1 - L/x1) iln: ((L/x1) (2.0e-15 + 1.5 eps) + eps) |iln| + 2.5 eps |d1|, d0 likewise with x0, both
           taken relative to max(|d1|, |d0|)
  block_suffix_excl   64 nthreads eps relative (its comment's promise for tiny terms; every partial sum is of positives)
Collectives are bit-identical to the order emulations below; div_small equals n // d.

FINDINGS (MI355X; the figures are profiles/math_helper_errors.json).  Every stated and every derived bar held at the first
measurement, so no derivation and no comment had to be corrected.  Closest to their bars: cmul 0.96 of eps sum|products| (the
bound is attained when both products round the same way), ftanh_half_small 1.38 ulp of 6e-17 + 1.5 ulp, fexp_tiny 0.89 ulp
of 1.5, dcerror_upper 2.8e-15 of the comment's 5e-15, planck_b 1.8 ulp of 4 on the Bernoulli branch.  Far inside: fsqrt
3.5e-15 of 2^-45 (v_rsq_f64 is better than the 2^-23 the comment assumes), layer_value 1.8e-15 of 2.9e-14 on the `any`
branch, hui_w_dw 1.4e-15 (w) and 7.3e-15 (dw) where the running-error bars allow 1.5e-13 and 1.2e-12 at their widest.
"""
import decimal
import functools
import os
import re
from decimal import Decimal as D
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")
PREC = 50
EPS = 2.0 ** -52
FDIV1 = 2.0 ** -46
FSQRT = 2.0 ** -45
WAVE = 64
N = 8191                        # points per scalar helper: no multiple of 64, the last wave runs with an inactive lane
BLOCK = 256


def hp(fn):
    """run fn under a PREC-digit decimal context"""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with decimal.localcontext() as ctx:
            ctx.prec = PREC
            ctx.Emax, ctx.Emin = 999999, -999999
            return fn(*a, **kw)
    return wrapped


def constant(name, header="mwrt_math.hip.h"):
    """a ``constexpr double NAME = value;`` of a device header, read from its text"""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr\s+double\s+%s\s*=\s*([-+0-9.eE]+)\s*;" % name, text)
    assert m, name
    return float(m.group(1))


EXP_SMALL_X = constant("EXP_SMALL_X")
EXP_TINY_X = constant("EXP_TINY_X")
PLANCK_SMALL_X = constant("PLANCK_SMALL_X")
LOGMEAN_SMALL_S = constant("LOGMEAN_SMALL_S", "mwrt_layer.hip.h")
LOGMEAN_MID_S = constant("LOGMEAN_MID_S", "mwrt_layer.hip.h")
SAME_D = 1e-09                  # |x1 - x0| below this: the layer value is x1 (mwrt_layer.hip.h:76, mwrt_tl_dev.hip.h:61)
Z_MAX = 0.1716 ** 2


def hui_coefficients():
    """{header: (a[7], b[7])} as decimal strings, from dcerror_upper (a0 = ..., b0 = ...) and hui_w_dw (a[7] = {...})"""
    num = r"[0-9]+\.[0-9]+"
    text = open(os.path.join(CSRC, "mwrt_math.hip.h")).read()
    body = text[text.index("dcerror_upper(double x, double y)"):]
    one = tuple([re.search(r"\b%s%d = (%s)" % (c, k, num), body).group(1) for k in range(7)] for c in "ab")
    text = open(os.path.join(CSRC, "mwrt_tl_dev.hip.h")).read()
    body = text[text.index("void hui_w_dw("):]
    two = tuple(re.findall(num, re.search(r"const double %s\[7\] = \{(.*?)\}" % c, body, flags=re.S).group(1)) for c in "ab")
    return {"mwrt_math.hip.h": one, "mwrt_tl_dev.hip.h": two}


# ---------------------------------------------------------------------------------------------------------------------
# scalar references: lists of Decimal from arrays of doubles
# ---------------------------------------------------------------------------------------------------------------------
def dec(x):
    return D(float(x))


@hp
def ref_exp(x):
    return [dec(v).exp() for v in x]


@hp
def ref_tanh_half(x):
    out = []
    for v in x:
        v = dec(v)
        if abs(v) < D("1e-8"):                      # 1 - e^-x would cancel: x/2 - x^3/24 + x^5/240 (next term 1e-48 relative)
            out.append(v / 2 - v ** 3 / 24 + v ** 5 / 240)
        else:
            e = (-v).exp()
            out.append((1 - e) / (1 + e))
    return out


@hp
def ref_two_atanh_over_s(z):
    """2 atanh(s) / s, s = sqrt z: through ln for z >= 1e-6, by the Taylor series 2 sum z^k / (2k + 1) in Fraction below"""
    out = []
    for v in z:
        if v >= 1e-6:
            s = dec(v).sqrt()
            out.append(((1 + s) / (1 - s)).ln() / s)
        else:
            f = Fraction(float(v))
            t = sum(2 * f ** k / (2 * k + 1) for k in range(10))          # z^10 <= 1e-60
            out.append(D(t.numerator) / D(t.denominator))
    return out


@hp
def ref_two_atanh_tail(z):
    out = []
    for v, full in zip(z, ref_two_atanh_over_s(z)):
        if v >= 1e-6:
            out.append((full - 2) / dec(v))
        else:
            f = Fraction(float(v))
            t = sum(2 * f ** (k - 1) / (2 * k + 1) for k in range(1, 11))
            out.append(D(t.numerator) / D(t.denominator))
    return out


@hp
def ref_sqrt(x):
    return [dec(v).sqrt() for v in x]


@hp
def ref_planck(x):
    return [1 / (dec(v).exp() - 1) for v in x]


# complex numbers as (re, im) pairs of Decimal
def c_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def c_recip(b):
    d = b[0] * b[0] + b[1] * b[1]
    return (b[0] / d, -b[1] / d)


def c_abs(a):
    return (a[0] * a[0] + a[1] * a[1]).sqrt()


@hp
def ref_crecip(re, im):
    return [c_recip((dec(a), dec(b))) for a, b in zip(re, im)]


@hp
def ref_cmul_cdiv(ar, ai, br, bi):
    """-> [(a b, a / b, bar of a b (re, im), bar of a / b (re, im))]"""
    out = []
    for a0, a1, b0, b1 in zip(ar, ai, br, bi):
        a, b = (dec(a0), dec(a1)), (dec(b0), dec(b1))
        c = c_recip(b)
        e = D(EPS)
        out.append((c_mul(a, b), c_mul(a, c),
                    (e * (abs(a[0] * b[0]) + abs(a[1] * b[1])), e * (abs(a[0] * b[1]) + abs(a[1] * b[0]))),
                    (4 * e * (abs(a[0] * c[0]) + abs(a[1] * c[1])), 4 * e * (abs(a[0] * c[1]) + abs(a[1] * c[0])))))
    return out


@hp
def ref_csqrt(re, im):
    """principal square root; the imaginary part carries the sign of Im z, -0.0 included"""
    out = []
    for x, y in zip(re, im):
        x, y = dec(x), dec(y)
        r = (x * x + y * y).sqrt()
        if x >= 0:
            a = ((r + x) / 2).sqrt()
            out.append((a, y / (2 * a)))
        else:
            b = ((r - x) / 2).sqrt()
            out.append((abs(y) / (2 * b), b.copy_sign(y)))
    return out


@hp
def ref_hui(zre, zim, header="mwrt_math.hip.h"):
    """the Hui rational at zh = (zre, zim) by plain complex Horner: [(w, dw, bar_w, bar_dw)], the bars absolute (docstring)"""
    a, b = hui_coefficients()[header]
    a = [D(c) for c in a]
    b = [D(c) for c in b] + [D(1)]
    out = []
    e = D(EPS)
    for x, y in zip(zre, zim):
        z = (dec(x), dec(y))
        az = c_abs(z)

        def horner(c):
            p, dp = (D(0), D(0)), (D(0), D(0))
            for ck in reversed(c):
                dp = c_mul(dp, z)
                dp = (dp[0] + p[0], dp[1] + p[1])
                p = c_mul(p, z)
                p = (p[0] + ck, p[1])
            pw = [D(1)]
            for _ in c[1:]:
                pw.append(pw[-1] * az)
            s = sum(ck * pw[k] for k, ck in enumerate(c))
            ds = sum(k * ck * pw[k - 1] for k, ck in enumerate(c) if k)
            return p, dp, s, ds
        p, dp, sp, dsp = horner(a)
        q, dq, sq, dsq = horner(b)
        iq = c_recip(q)
        w = c_mul(p, iq)
        wdq = c_mul(w, dq)
        dw = c_mul((dp[0] - wdq[0], dp[1] - wdq[1]), iq)
        aw, aq = c_abs(w), c_abs(q)
        bar_w = aw * (20 * e * (sp / c_abs(p) + sq / aq) + 5 * e)
        bar_dw = (20 * e * dsp + aw * 20 * e * dsq + c_abs(dq) * bar_w + 2 * e * (c_abs(dp) + c_abs(wdq))) / aq + 5 * e * c_abs(dw)
        out.append((w, dw, bar_w, bar_dw))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the layer rule
# ---------------------------------------------------------------------------------------------------------------------
BRANCHES = ("negative", "same", "zero", "small", "mid", "any")
REL_S = FDIV1 + 1.5 * EPS
BAR_LV = {"small": 2 * 0.0101 * REL_S + 1.1e-18 + 1.5 * EPS,
          "mid": 2 * 0.1763 * REL_S + FDIV1 + 14 * EPS + 7.7e-17 + 2 * EPS,
          "any": 2 * FDIV1 + 3.5 * EPS}
BAR_TL = {"small": 3 * EPS, "any": 6.8 * EPS + 5e-16}
BAR_TL_PARTIAL_SMALL = 4 * EPS
SWITCH_SLACK = 1e-12


def layer_branch(x1, x0):
    """the branch of the layer rule a pair of doubles takes, restated from mwrt_layer.hip.h / mwrt_tl_dev.hip.h:
    negative end -> 0 and neg; |d| < 1e-9 -> x1; zero end -> sm/2 or 0; else the log-mean, named by its |s| band"""
    x1, x0 = float(x1), float(x0)
    if x0 < 0.0 or x1 < 0.0:
        return "negative"
    if abs(x1 - x0) < SAME_D:
        return "same"
    if x0 == 0.0 or x1 == 0.0:
        return "zero"
    s = abs((x1 - x0) / (x1 + x0))
    return "small" if s <= LOGMEAN_SMALL_S else ("mid" if s <= LOGMEAN_MID_S else "any")


@hp
def ref_layer(x1, x0, zeroflg=True):
    """-> [(branch, value, d/dx1, d/dx0)] in Decimal.  The partials are those of the branch taken: (0, 0), (1, 0),
    (1/2, 1/2) or (0, 0), and the log-mean's L (1 - L/x1)/(x1 - x0) ... written through ln"""
    out = []
    for a, b in zip(x1, x0):
        br = layer_branch(a, b)
        a, b = dec(a), dec(b)
        if br == "negative":
            out.append((br, D(0), D(0), D(0)))
        elif br == "same":
            out.append((br, a, D(1), D(0)))
        elif br == "zero":
            h = D("0.5") if zeroflg else D(0)                  # (one end is 0: the half sum is a double, taken exactly)
            out.append((br, dec(0.5 * (float(a) + float(b))) if zeroflg else D(0), h, h))
        else:
            ln = (a / b).ln()
            L = (a - b) / ln
            out.append((br, L, (1 - L / a) / ln, (L / b - 1) / ln))
    return out


def exact_abs_s(x1, x0):
    x1, x0 = Fraction(float(x1)), Fraction(float(x0))
    return abs((x1 - x0) / (x1 + x0))


def wave_branches(x1, x0, live, lanes_per_thread=1):
    """the series branch each wave of layer_value / layer_value4 takes: the widest band among its live, non-special
    lanes (a wave with none takes "small"); (lo, hi) names where a lane within SWITCH_SLACK of a switch leaves it open.
    lanes_per_thread = 4: thread t holds elements 4t .. 4t+3 and votes for all four, live read at its first element."""
    n = len(x1)
    order = {"small": 0, "mid": 1, "any": 2}
    names = ("small", "mid", "any")
    per_wave = WAVE * lanes_per_thread
    out = []
    for w0 in range(0, n, per_wave):
        lo = hi = 0
        for i in range(w0, min(n, w0 + per_wave)):
            if not live[(i // lanes_per_thread) * lanes_per_thread]:
                continue
            br = layer_branch(x1[i], x0[i])
            if br not in order:
                continue
            s = exact_abs_s(x1[i], x0[i])
            l = h = order[br]
            for k, t in enumerate((LOGMEAN_SMALL_S, LOGMEAN_MID_S)):
                if abs(s / Fraction(t) - 1) <= Fraction(SWITCH_SLACK):
                    l, h = min(l, k), max(h, k + 1)
            lo, hi = max(lo, l), max(hi, h)
        out.append((names[lo], names[hi]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# collectives: the order of the device sums, in float64
# ---------------------------------------------------------------------------------------------------------------------
def emu_block_sum(v, nthreads):
    """block_sum (mwrt_math.hip.h): butterfly by xor 32, 16, .., 1 within each wave, then the waves in index order"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, nthreads // WAVE, WAVE).copy()
    lane = np.arange(WAVE)
    o = WAVE // 2
    while o:
        v = v + v[..., lane ^ o]
        o >>= 1
    s = np.zeros(v.shape[0])
    for w in range(v.shape[1]):
        s = s + v[:, w, 0]
    return np.repeat(s, nthreads)


def emu_block_scan(v, nthreads):
    """block_scan (mwrt_tl_dev.hip.h): up-shuffles by 1, 2, .., 32, then the offsets of the waves below, in index order.
    -> (inclusive prefix, total)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, nthreads // WAVE, WAVE).copy()
    o = 1
    while o < WAVE:
        u = v.copy()
        u[..., o:] = v[..., o:] + v[..., :-o]
        v = u
        o <<= 1
    wsum = v[..., WAVE - 1]
    off = np.zeros(wsum.shape)
    tot = np.zeros(wsum.shape[0])
    for w in range(wsum.shape[1]):
        off[:, w + 1:] = off[:, w + 1:] + wsum[:, w:w + 1]         # off += (w < wave) ? x : 0, in the order of w
        tot = tot + wsum[:, w]
    return (v + off[..., None]).ravel(), np.repeat(tot, nthreads)


def emu_block_suffix_excl(v, nthreads):
    """block_suffix_excl: down-shuffles by 1, 2, .., 32 (inclusive suffix within the wave), the next lane's value, then
    the totals of the waves above from the top down"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, nthreads // WAVE, WAVE).copy()
    o = 1
    while o < WAVE:
        u = v.copy()
        u[..., :-o] = v[..., :-o] + v[..., o:]
        v = u
        o <<= 1
    wsum = v[..., 0]
    nxt = np.zeros(v.shape)
    nxt[..., :-1] = v[..., 1:]
    off = np.zeros(wsum.shape)
    for wave in range(wsum.shape[1]):
        for w in range(wsum.shape[1] - 1, wave, -1):
            off[:, wave] = off[:, wave] + wsum[:, w]
    return (nxt + off[..., None]).ravel()


def emu_row16_max(v):
    v = np.asarray(v, dtype=np.float64).astype(np.float32).reshape(-1, 16)
    return np.repeat(v.max(axis=1), 16).astype(np.float64)


@hp
def exact_suffix_excl(v, nthreads):
    """the true exclusive suffix sums per workgroup, in Decimal"""
    out = []
    for g in range(0, len(v), nthreads):
        acc, part = D(0), []
        for x in reversed(v[g:g + nthreads]):
            part.append(acc)
            acc += dec(x)
        out.extend(reversed(part))
    return out


def pad(v, nthreads, fill=0.0):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, np.full(-len(v) % nthreads, fill)])


# ---------------------------------------------------------------------------------------------------------------------
# input sets (seeded; the GPU tests, the CPU self-checks and tools/math_helper_errors.py all use these)
# ---------------------------------------------------------------------------------------------------------------------
def around(x, k=4):
    """x and the k doubles either side of it"""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return [float(v) for v in out]


def fill(points, n, rng, lo, hi, log=False):
    """the listed points first, then a seeded random fill of [lo, hi] (log-uniform in magnitude if log) up to n"""
    points = np.asarray(points, dtype=np.float64)
    m = n - len(points)
    assert m > 0
    r = np.exp(rng.uniform(np.log(lo), np.log(hi), m)) if log else rng.uniform(lo, hi, m)
    return np.concatenate([points, r])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the input arrays of one helper (tuple of float64 arrays of equal length, at most 8192 points)"""
    rng = np.random.default_rng([20240611, sum(map(ord, name))])
    if name == "fexp_small":
        pts = [0.0, -0.0, -EXP_SMALL_X, EXP_SMALL_X] + [v for v in around(EXP_TINY_X) + around(-EXP_TINY_X)]
        pts += [v for v in around(EXP_SMALL_X) if abs(v) <= EXP_SMALL_X] + [v for v in around(-EXP_SMALL_X) if abs(v) <= EXP_SMALL_X]
        x = fill(pts + [1e-300, -1e-300, 1e-20, -1e-20], N, rng, -EXP_SMALL_X, EXP_SMALL_X)
        return (x,)
    if name == "fexp_tiny":
        pts = [0.0, -0.0] + [v for s in (1, -1) for v in around(s * EXP_TINY_X) if abs(v) <= EXP_TINY_X]
        return (fill(pts + [1e-300, -1e-300, 1e-20, -1e-20], N, rng, -EXP_TINY_X, EXP_TINY_X),)
    if name in ("ftanh_half_small", "ftanh_half_tiny"):
        top = EXP_SMALL_X if name.endswith("small") else EXP_TINY_X
        pts = [0.0, top] + [v for v in around(top) if v <= top] + [v for v in around(EXP_TINY_X) if v <= top]
        pos = np.concatenate([fill(pts, 3000, rng, 0.0, top), np.exp(rng.uniform(np.log(1e-300), np.log(top), 1095))])
        return (np.concatenate([pos, -pos, [0.0]]),)                         # x, -x (oddness, -0.0 included), 8191 in all
    if name == "two_atanh_tail":
        pts = [0.0, Z_MAX, 1e-6] + around(1e-6)
        return (np.concatenate([fill(pts, 6000, rng, 0.0, Z_MAX), np.exp(rng.uniform(np.log(1e-30), np.log(Z_MAX), N - 6000))]),)
    if name == "fsqrt":
        x = np.concatenate([rng.uniform(100.0 / 50.0, 350.0 / 16.0, 2000), fill([1e-16, 1e8, 1.0, 2.0, 4.0], N - 2000, rng, 1e-16, 1e8, log=True)])
        return (x,)
    if name in ("csqrt_principal", "crecip"):
        lo, hi = (1e-4, 1e4) if name == "csqrt_principal" else (1e-6, 1e4)
        mod = np.exp(rng.uniform(np.log(lo), np.log(hi), 2040))
        ph = rng.uniform(-np.pi, np.pi, 2040)
        ph[:680] = rng.uniform(-np.pi / 2, np.pi / 2, 680)                   # Re > 0: what the speed-dependent shape feeds it
        re, im = mod * np.cos(ph), mod * np.sin(ph)
        edge_re = [0.0, -0.0, 1.0, -1.0, 1e-4, -1e-4, 1e4, -1e4]
        edge_im = [0.0, -0.0, 1.0, -1.0, 1e-4, -1e-4, 1e4, -1e4]
        er, ei = np.meshgrid(edge_re, edge_im)
        keep = ~((er == 0) & (ei == 0))                                      # z = 0 is outside the domain
        re, im = np.concatenate([er[keep], re]), np.concatenate([ei[keep], im])
        # z and conj z, then -conj z ... : 4 * 2047 + 3 = 8191
        re = np.concatenate([re[:2047], re[:2047], -re[:2047], -re[:2047], [1.0, 2.0, 3.0]])
        im = np.concatenate([im[:2047], -im[:2047], im[:2047], -im[:2047], [1.0, -2.0, 0.0]])
        return (re, im)
    if name == "dcerror_upper":                                             # the same points as hui_w_dw: zh = (|y|, -x)
        zr, zi = inputs("hui_w_dw")
        return (-zi, zr)
    if name == "hui_w_dw":
        mod = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(100.0), 4000)), rng.uniform(0.0, 100.0, N - 4000 - 8)])
        ph = rng.uniform(-np.pi / 2, np.pi / 2, len(mod))
        zr = np.concatenate([mod * np.cos(ph), [0.0, 0.0, 100.0, 1e-6, 0.0, 3.0, 0.0, 0.0]])
        zi = np.concatenate([mod * np.sin(ph), [100.0, -100.0, 0.0, 0.0, 1e-6, 0.0, 3.0, -3.0]])
        return (zr, zi)
    if name == "cmul_cdiv":
        def comp():
            return np.exp(rng.uniform(np.log(1e-6), np.log(1e4), N)) * rng.choice([-1.0, 1.0], N)
        ar, ai, br, bi = comp(), comp(), comp(), comp()
        ai[:16] = 0.0
        bi[8:24] = 0.0
        ar[24:32] = 0.0
        return (ar, ai, br, bi)
    if name == "planck_bernoulli":
        hk = 0.0479924307                                                    # h / k in K / GHz
        x = np.concatenate([hk * np.exp(rng.uniform(0.0, np.log(1000.0), 3000)) / rng.uniform(100.0, 350.0, 3000),
                            np.exp(rng.uniform(np.log(1e-6), np.log(PLANCK_SMALL_X), 1000))])
        x = x[x <= PLANCK_SMALL_X]
        pts = [v for v in around(PLANCK_SMALL_X) if v <= PLANCK_SMALL_X] + [hk / 350.0, 1e-6]
        x = np.concatenate([pts, x])
        return (x[:len(x) - (len(x) % WAVE == 0)],)
    if name == "planck_general":
        xb = inputs("planck_bernoulli")[0]
        x = np.concatenate([xb, around(PLANCK_SMALL_X), rng.uniform(PLANCK_SMALL_X, 0.5, 1500), rng.uniform(0.5, 5.0, 500), [5.0]])
        out = np.empty(len(x) + -(-len(x) // 63))
        pivot = np.arange(len(out)) % WAVE == 0                              # lane 0 of every wave holds 0.05
        out[pivot], out[~pivot] = 0.05, x
        return (out[:len(out) - (len(out) % WAVE == 0)],)
    if name == "layer":
        return layer_inputs(rng)
    if name == "div_small":
        ns, ds = [], []
        for d in range(1, 1025):
            m = np.arange(0, 65536, d)
            nn = np.unique(np.concatenate([m, m[1:] - 1, [0, 65535]]))
            ns.append(nn)
            ds.append(np.full(len(nn), d))
        return (np.concatenate(ns).astype(np.float64), np.concatenate(ds).astype(np.float64))
    raise KeyError(name)


def layer_inputs(rng):
    """(x1, x0, live): whole waves in each series branch, waves of identical lanes with one lane in another band, a mixed
    stretch with the special cases and the switches, lanes that are not live.  8188 elements (a multiple of 4 for
    layer_value4, no multiple of 64); waves are 64 consecutive elements."""
    def pairs(n, smin, smax):
        x0 = np.exp(rng.uniform(np.log(1e-6), np.log(1e2), n))               # large enough that |d| >= 1e-9
        s = rng.uniform(smin, smax, n) * rng.choice([-1.0, 1.0], n)
        return x0 * (1 + s) / (1 - s), x0
    x1, x0 = [], []

    def add(a, b):
        x1.append(np.asarray(a, dtype=np.float64))
        x0.append(np.asarray(b, dtype=np.float64))
    # waves 0-31: small only (x0 large enough that |d| >= 1e-9); 32-47: mid only; 48-63: any, ratios up to 1e6
    a0 = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), 32 * WAVE))
    s = rng.uniform(1e-4, 0.17, 32 * WAVE) * rng.choice([-1.0, 1.0], 32 * WAVE)
    add(a0 * (1 + s) / (1 - s), a0)
    add(*pairs(16 * WAVE, 0.18, 0.59))
    a0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e2), 16 * WAVE))
    add(a0 * np.exp(rng.uniform(np.log(4.1), np.log(1e6), 16 * WAVE) * rng.choice([-1.0, 1.0], 16 * WAVE)), a0)
    # waves 64-69: identical lanes (1.02, 1.0), one lane moved: to mid, to any; identical mid lanes with one any, one small;
    # identical any lanes with one small, one mid
    for base, odd in (((1.02, 1.0), (2.0, 1.0)), ((1.02, 1.0), (9.0, 1.0)), ((2.0, 1.0), (9.0, 1.0)), ((2.0, 1.0), (1.02, 1.0)),
                      ((9.0, 1.0), (1.02, 1.0)), ((9.0, 1.0), (2.0, 1.0))):
        a, b = np.full(WAVE, base[0]), np.full(WAVE, base[1])
        a[37], b[37] = odd
        add(a, b)
    # waves 70-77: the special cases and the switches among ordinary lanes
    sp1, sp0 = [], []
    for v in (0.0, 1e-3, 1.0):
        sp1 += [-1e-3, v, -1.0, -0.0]
        sp0 += [v, -1e-3, -2.0, -1e-300]                                     # negative ends (-0.0 is not negative)
    for v in (0.0, -0.0):
        sp1 += [v, 0.5, 1e-12, v]
        sp0 += [0.5, v, v, 1e-3]                                             # zero ends
    sp1 += [0.0, 1.0, 1.0 + 5e-10, 5e-10, 1e-12]
    sp0 += [0.0, 1.0, 1.0, 0.0, 7e-10]                                       # same (|d| < 1e-9), some with a zero end
    for base in (1.0, 3e-7):
        for d in around(SAME_D):                                             # |d| = 1e-9 +- 4 ulp, both signs
            sp1 += [base + d, base]
            sp0 += [base, base + d]
    sp1 += around(SAME_D)                                                    # ... and exactly, against a zero end
    sp0 += [0.0] * 9
    for t in (LOGMEAN_SMALL_S, LOGMEAN_MID_S):                               # |s| at the series switches
        for sv in around(t):
            sp1 += [float((1 + sv) / (1 - sv)), 1.0]
            sp0 += [1.0, float((1 + sv) / (1 - sv))]
    for m in (0.70710678118654752440, 1.41421356237309504880):               # the mantissa selects of flog / log_mean_any
        for v in around(m):
            sp1 += [v, 1.0, 8.0 * v]
            sp0 += [1.0, v, 1.0]
    k = 8 * WAVE - len(sp1)
    assert k > 0
    a0 = np.exp(rng.uniform(np.log(1e-12), np.log(1e2), k))
    r = np.exp(rng.uniform(np.log(1.0001), np.log(1e3), k) * rng.choice([-1.0, 1.0], k))
    mix1, mix0 = np.concatenate([sp1, a0 * r]), np.concatenate([sp0, a0])
    perm = rng.permutation(8 * WAVE)
    add(mix1[perm], mix0[perm])
    # waves 78-127 (the last one short): small lanes; in every fourth wave some lanes are NOT live and hold a negative end
    # or a far ratio: neither may set neg or move the wave's vote
    rest = 8188 - sum(len(a) for a in x1)
    a0 = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), rest))
    s = rng.uniform(1e-4, 0.17, rest) * rng.choice([-1.0, 1.0], rest)
    b1 = a0 * (1 + s) / (1 - s)
    live = np.ones(8188)
    first = 8188 - rest
    dead = np.arange(first + 8, 8188, 4 * WAVE)
    dead = np.concatenate([dead, dead + 1, dead + 2, dead + 3])              # whole quads: layer_value4 reads live once per thread
    add(b1, a0)
    x1a, x0a = np.concatenate(x1), np.concatenate(x0)
    live[dead] = 0.0
    x1a[dead[::2]] = -1.0
    x1a[dead[1::2]] = 1e5 * x0a[dead[1::2]]
    return (x1a, x0a, live)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def ulp(ref):
    return float(np.spacing(abs(float(ref)))) if ref != 0 else 5e-324


@hp
def errors(dev, ref):
    """|dev - ref| per point as floats, exact in Decimal (dev: doubles, ref: Decimals)"""
    return np.array([float(abs(dec(d) - r)) for d, r in zip(dev, ref)])


def bar_of(ref, rel=0.0, nulp=0.0):
    return np.array([rel * abs(float(r)) + nulp * ulp(r) for r in ref])


def check(name, dev, ref, bar, source, report=None):
    """-> dict(points, worst = max err / bar, max_rel, max_ulp, bar ...).  `bar`: absolute per point.  A point with bar 0
    must be met exactly.  `report`: a dict the figures are stored in under `name` (the tool's JSON, the tests' prints)."""
    assert len(dev) == len(ref) == len(bar) and np.all(np.isfinite(np.asarray(dev, dtype=np.float64))), name
    err = errors(dev, ref)
    mag = np.array([abs(float(r)) for r in ref])
    nz = mag > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    ulps = np.array([ulp(r) for r in ref])
    row = dict(points=int(len(dev)), worst_err_over_bar=float(ratio.max()), max_rel=float((err[nz] / mag[nz]).max()) if nz.any() else 0.0,
               max_ulp=float((err / ulps).max()), max_abs_where_ref_is_0=float(err[~nz].max()) if (~nz).any() else 0.0,
               bar_rel_max=float((bar[nz] / mag[nz]).max()) if nz.any() else 0.0, bar_ulp_max=float((bar / ulps).max()), bar_from=source)
    if report is not None:
        report[name] = row
    print("%-28s n=%5d  max rel %.3e  max ulp %.3f  worst err/bar %.3f  (bar <= %.3e rel; %s)" % (
        name, row["points"], row["max_rel"], row["max_ulp"], row["worst_err_over_bar"], row["bar_rel_max"], source))
    return row
