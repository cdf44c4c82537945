"""tests/math_reference.py against itself (no GPU): the Decimal references agree with numpy / libm and, where installed,
with mpmath; the coefficient reader finds the Hui coefficients in both headers; the order emulations reproduce a case worked
by hand; the layer inputs reach every branch of the restated layer rule."""
import math

import numpy as np
import pytest

import math_reference as mr


def ulps(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def f(dec_list):
    return np.array([float(v) for v in dec_list])


def test_references_agree_with_libm_to_2_ulp():
    rng = np.random.default_rng(1)
    x = rng.uniform(-0.125, 0.125, 300)
    assert ulps(f(mr.ref_exp(x)), np.exp(x)).max() <= 2
    assert ulps(f(mr.ref_tanh_half(x)), np.tanh(0.5 * x)).max() <= 2
    assert ulps(f(mr.ref_tanh_half([1e-12, -3e-9, 0.0])), np.tanh(0.5 * np.array([1e-12, -3e-9, 0.0]))).max() <= 2
    y = np.exp(rng.uniform(np.log(1e-16), np.log(1e8), 300))
    assert ulps(f(mr.ref_sqrt(y)), np.sqrt(y)).max() <= 2
    z = rng.uniform(1e-3, mr.Z_MAX, 300)
    s = np.sqrt(z)
    assert ulps(f(mr.ref_two_atanh_over_s(z)), 2 * np.arctanh(s) / s).max() <= 2
    # the tail itself cancels in double ((2 atanh(s)/s - 2)/z): compare with its series instead, on both sides of the 1e-6 switch
    zz = np.array([0.0, 1e-30, 1e-9, 0.99e-6, 1e-6, 1.01e-6, 1e-4])
    series = sum(2 * zz ** (k - 1) / (2 * k + 1) for k in range(1, 8))
    assert ulps(f(mr.ref_two_atanh_tail(zz)), series).max() <= 2
    p = np.exp(rng.uniform(np.log(1e-4), np.log(5.0), 300))
    assert ulps(f(mr.ref_planck(p)), 1 / np.expm1(p)).max() <= 2
    re, im = rng.standard_normal(300) * 10, rng.standard_normal(300) * 10
    got = mr.ref_csqrt(re, im)
    want = np.sqrt(re + 1j * im)
    assert ulps(f([g[0] for g in got]), want.real).max() <= 2 and ulps(f([g[1] for g in got]), want.imag).max() <= 2
    got = mr.ref_crecip(re, im)
    want = 1 / (re + 1j * im)
    assert ulps(f([g[0] for g in got]), want.real).max() <= 2 and ulps(f([g[1] for g in got]), want.imag).max() <= 2


def test_csqrt_reference_signed_zeros():
    got = mr.ref_csqrt([-4.0, -4.0, 4.0, 4.0, 0.0, 0.0], [0.0, -0.0, 0.0, -0.0, 2.0, -2.0])
    assert [(float(a), float(b)) for a, b in got] == [(0.0, 2.0), (0.0, -2.0), (2.0, 0.0), (2.0, -0.0), (1.0, 1.0), (1.0, -1.0)]
    assert [math.copysign(1.0, float(b)) for _, b in got] == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0]


def test_hui_reference():
    c = mr.hui_coefficients()
    assert c["mwrt_math.hip.h"] == c["mwrt_tl_dev.hip.h"]
    a, b = c["mwrt_math.hip.h"]
    assert len(a) == 7 and len(b) == 7 and a[0] == "122.607931777104326" and b[6] == "10.479857114260399" and a[6] == "0.564189583562615"
    # the rational is w(z) = exp(-z^2) erfc(-i z) to ~1e-6 (zh = -i z): on the imaginary axis w(i y) = exp(y^2) erfc(y)
    y = np.array([0.0, 0.3, 1.0, 2.5, 10.0])
    got = mr.ref_hui(y, np.zeros(5))
    want = np.array([math.exp(v * v) * math.erfc(v) for v in y])
    assert np.abs(f([g[0][0] for g in got]) - want).max() < 2e-6 and all(g[0][1] == 0 for g in got)
    # the derivative is that of the rational: central difference of the reference itself, along the real zh axis
    h = 1e-6
    up, dn, mid = mr.ref_hui([1.0 + h], [0.5]), mr.ref_hui([1.0 - h], [0.5]), mr.ref_hui([1.0], [0.5])
    for k in (0, 1):
        assert abs(float((up[0][0][k] - dn[0][0][k])) / (2 * h) - float(mid[0][1][k])) < 1e-9
    assert all(float(g[2]) > 0 and float(g[3]) > 0 for g in got)


def test_layer_reference_and_branch_reach():
    x1, x0, live = mr.inputs("layer")
    assert len(x1) == 8188 and len(x1) % 4 == 0 and len(x1) % 64 != 0 and len(x1) <= 8192
    count = {b: 0 for b in mr.BRANCHES}
    for a, b in zip(x1, x0):
        count[mr.layer_branch(a, b)] += 1
    print(count)
    assert all(count[b] > 0 for b in mr.BRANCHES), count
    # ... and among the live lanes, with both kinds of zero end and both orders of a negative end
    alive = {b: 0 for b in mr.BRANCHES}
    for a, b, l in zip(x1, x0, live):
        alive[mr.layer_branch(a, b)] += int(l != 0)
    assert all(alive[b] > 0 for b in mr.BRANCHES), alive
    # waves: some take each band outright, some are left open by a lane at a switch
    waves = mr.wave_branches(x1, x0, live)
    assert {("small", "small"), ("mid", "mid"), ("any", "any")} <= set(waves) and len(waves) == 128
    assert all(w == ("small", "small") for w in waves[78:]), "a lane that is not live moved its wave's vote"
    r = mr.ref_layer([2.0, 1.0, -1.0, 0.0, 3.0, 1.0 + 1e-12], [1.0, 2.0, 1.0, 3.0, 0.0, 1.0])
    assert abs(float(r[0][1]) - 1 / math.log(2.0)) < 1e-15 and abs(float(r[1][1]) - 1 / math.log(2.0)) < 1e-15
    assert [q[0] for q in r] == ["mid", "mid", "negative", "zero", "zero", "same"]
    assert (float(r[3][1]), float(r[3][2]), float(r[3][3])) == (1.5, 0.5, 0.5) and (float(r[5][2]), float(r[5][3])) == (1.0, 0.0)
    z = mr.ref_layer([0.0], [3.0], zeroflg=False)[0]
    assert (float(z[1]), float(z[2]), float(z[3])) == (0.0, 0.0, 0.0)
    # the partials are the log-mean's: central differences of the reference
    h = 1e-7
    L = lambda a, b: float(mr.ref_layer([a], [b])[0][1])
    d = mr.ref_layer([2.0], [0.7])[0]
    assert abs((L(2.0 + h, 0.7) - L(2.0 - h, 0.7)) / (2 * h) - float(d[2])) < 1e-8
    assert abs((L(2.0, 0.7 + h) - L(2.0, 0.7 - h)) / (2 * h) - float(d[3])) < 1e-8


def test_input_sets():
    for name in ("fexp_small", "fexp_tiny", "ftanh_half_small", "ftanh_half_tiny", "two_atanh_tail", "fsqrt", "crecip", "cmul_cdiv",
                 "csqrt_principal", "dcerror_upper", "hui_w_dw", "planck_bernoulli", "planck_general"):
        x = mr.inputs(name)
        assert all(len(a) == len(x[0]) for a in x) and len(x[0]) <= 8192 and len(x[0]) % 64 != 0, (name, len(x[0]))
        assert all(np.isfinite(a).all() for a in x), name
    assert np.abs(mr.inputs("fexp_small")[0]).max() == mr.EXP_SMALL_X and np.abs(mr.inputs("fexp_tiny")[0]).max() == mr.EXP_TINY_X
    t = mr.inputs("ftanh_half_small")[0]
    assert t.max() == mr.EXP_SMALL_X and t.min() == -mr.EXP_SMALL_X
    z = mr.inputs("two_atanh_tail")[0]
    assert z.min() == 0.0 and z.max() == mr.Z_MAX
    b = mr.inputs("planck_bernoulli")[0]
    assert b.max() == mr.PLANCK_SMALL_X and b.min() > 0
    g = mr.inputs("planck_general")[0]
    assert np.all(g[::64] == 0.05) and g.max() == 5.0 and (g == np.nextafter(mr.PLANCK_SMALL_X, 1.0)).any()
    re, im = mr.inputs("csqrt_principal")
    assert not ((re == 0) & (im == 0)).any() and (mr.inputs("fsqrt")[0] > 0).all()
    zr, zi = mr.inputs("hui_w_dw")
    assert (zr >= 0).all() and np.hypot(zr, zi).max() <= 100.0 * (1 + 1e-15)
    n, d = mr.inputs("div_small")
    for dd in (1, 7, 64, 1000, 1024):
        got = set(n[d == dd].astype(int).tolist())
        m = set(range(0, 65536, dd))
        assert {0, 65535} <= got and m <= got and {v - 1 for v in m if v} <= got


def test_order_emulations_on_a_hand_worked_case():
    """128 elements, two waves, v[i] = i + 1 for i < 64 and 1 for the rest: every partial sum is an exact integer, so the
    expected values are the triangular numbers; then three-term cases where the ORDER decides the rounding"""
    i = np.arange(64.0)
    v = np.concatenate([i + 1, np.ones(64)])
    s = mr.emu_block_sum(v, 128)
    assert np.all(s == 2080.0 + 64.0) and len(s) == 128
    p, t = mr.emu_block_scan(v, 128)
    assert np.array_equal(p[:64], (i + 1) * (i + 2) / 2) and np.array_equal(p[64:], 2080.0 + i + 1) and np.all(t == 2144.0)
    x = mr.emu_block_suffix_excl(v, 128)
    assert np.array_equal(x[64:], 63.0 - i) and x[127] == 0.0
    assert np.array_equal(x[:64], 2080.0 - (i + 1) * (i + 2) / 2 + 64.0) and x[63] == 64.0
    # the order matters where rounding does: three terms that do not associate
    w = np.zeros(128)
    w[0], w[1], w[64] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert mr.emu_block_sum(w, 128)[0] == 1.0                              # (1 + 2^-53) rounds to 1, then + 2^-53 again
    w[0], w[1], w[2] = 2.0 ** -53, 2.0 ** -53, 0.0
    w[64] = 1.0
    assert mr.emu_block_sum(w, 128)[0] == 1.0 + 2.0 ** -52                 # the two small terms meet first
    assert mr.emu_block_suffix_excl(w, 128)[0] == 1.0                      # lane 0: 2^-53 (lane 1) + 1 (the wave above) -> 1
    assert np.array_equal(mr.emu_row16_max(np.arange(32.0)), np.repeat([15.0, 31.0], 16))
    tr = mr.exact_suffix_excl([1.0, 1e-300, 1e-300], 3)
    assert [str(tr[2]), float(tr[1])] == ["0", 1e-300] and float(tr[0]) == 2e-300


def test_against_mpmath():
    mp = pytest.importorskip("mpmath")
    with mp.workdps(70):                  # (2 atanh(s)/s - 2)/z loses its leading digits in any arithmetic that forms it so
        _against_mpmath(mp)


def _against_mpmath(mp):
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.125, 0.125, 50)
    tol = mp.mpf(10) ** -40

    def close(dec_value, m):
        return abs(mp.mpf(str(dec_value)) - m) <= tol * max(abs(m), mp.mpf(10) ** -300)
    assert all(close(a, mp.exp(mp.mpf(float(v)))) for a, v in zip(mr.ref_exp(x), x))
    assert all(close(a, mp.tanh(mp.mpf(float(v)) / 2)) for a, v in zip(mr.ref_tanh_half(x), x))
    z = np.concatenate([rng.uniform(0, mr.Z_MAX, 40), [1e-9, 1e-7, 1e-6, 2e-6]])
    for a, v in zip(mr.ref_two_atanh_tail(z), z):
        s = mp.sqrt(mp.mpf(float(v)))
        assert close(a, (2 * mp.atanh(s) / s - 2) / mp.mpf(float(v)))
    p = np.exp(rng.uniform(np.log(1e-4), np.log(5.0), 50))
    assert all(close(a, 1 / mp.expm1(mp.mpf(float(v)))) for a, v in zip(mr.ref_planck(p), p))
    re, im = rng.standard_normal(50), rng.standard_normal(50)
    for (a, b), u, v in zip(mr.ref_csqrt(re, im), re, im):
        r = mp.sqrt(mp.mpc(float(u), float(v)))
        assert close(a, r.real) and close(b, r.imag)
    for (br, L, d1, d0), u, v in zip(mr.ref_layer(np.abs(re) + 0.1, np.abs(im) + 0.1), np.abs(re) + 0.1, np.abs(im) + 0.1):
        if br in ("small", "mid", "any"):
            assert close(L, (mp.mpf(float(u)) - mp.mpf(float(v))) / mp.log(mp.mpf(float(u)) / mp.mpf(float(v))))
