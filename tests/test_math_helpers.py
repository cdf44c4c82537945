"""Every device arithmetic helper on its own arguments, through mwrt_selftest_helpers, against the 50-digit references of
tests/math_reference.py (domains, bars and their derivations: that module's docstring).  The bars come from the accuracy
claims in the helpers' own comments or are derived there; the figures each test prints are those
tools/math_helper_errors.py writes to profiles/math_helper_errors.json."""
import numpy as np
import pytest

import math_helpers_device as mh
import math_reference as mr
from mwr_fast_forward_operators_and_lbls_amd import _native

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", sorted(mh.CHECKS))
def test_helper_meets_its_bar(gpu_ctx, name):
    for row in mh.CHECKS[name](gpu_ctx):
        assert row["worst_err_over_bar"] <= 1.0, row


def test_exp_and_tanh_exact_properties(gpu_ctx):
    for name in ("fexp_small", "fexp_tiny"):
        x = mr.inputs(name)[0]
        (o, o2, _, _), _ = mh.run(gpu_ctx, name, (x,))
        assert np.all(o[x == 0] == 1.0) and (x == 0).sum() >= 2, name
        if name == "fexp_small":
            assert np.array_equal(bits(o), bits(o2)), "loop_invariant_vgpr(c0) changed bits"
    for name in ("ftanh_half_small", "ftanh_half_tiny"):
        x = mr.inputs(name)[0]
        (o, o2, _, _), _ = mh.run(gpu_ctx, name, (x,))
        assert np.all(o[x == 0] == 0.0), name
        h = (len(x) - 1) // 2
        assert np.array_equal(x[:h], -x[h:2 * h])
        assert np.array_equal(bits(o[:h]), bits(-o[h:2 * h])), name + " is not odd bit for bit"
        if name == "ftanh_half_small":
            assert np.array_equal(bits(o), bits(o2)), "loop_invariant_vgpr(c0) changed bits"


def test_csqrt_principal_signs_and_conjugate(gpu_ctx):
    re, im = mr.inputs("csqrt_principal")
    (ore, oim, _, _), _ = mh.run(gpu_ctx, "csqrt_principal", (re, im))
    assert np.all(ore >= 0) and not np.signbit(ore).any()
    assert np.array_equal(np.signbit(oim), np.signbit(im)), "sign(Im sqrt z) != sign(Im z)"
    assert np.signbit(im[im == 0]).any() and (~np.signbit(im[im == 0])).any() and (re[im == 0] < 0).any()
    q = 2047                                           # z, conj z, -conj z, -z
    assert np.array_equal(re[:q], re[q:2 * q]) and np.array_equal(im[:q], -im[q:2 * q])
    assert np.array_equal(bits(ore[:q]), bits(ore[q:2 * q])) and np.array_equal(bits(oim[:q]), bits(-oim[q:2 * q]))
    assert np.array_equal(bits(ore[2 * q:3 * q]), bits(ore[3 * q:4 * q])) and np.array_equal(bits(oim[2 * q:3 * q]), bits(-oim[3 * q:4 * q]))


def test_hui_schemes_agree(gpu_ctx):
    """dcerror_upper's quadratic recurrence and hui_w_dw's complex Horner evaluate one rational: within the sum of their bars"""
    (re, im, _, _), _ = mh.run(gpu_ctx, "dcerror_upper", mr.inputs("dcerror_upper"))
    (wre, wim, _, _), _ = mh.run(gpu_ctx, "hui_w_dw", mr.inputs("hui_w_dw"))
    ref = mh.reference("hui")
    mag = np.array([float(mr.c_abs(r[0])) for r in ref])
    bar = 5e-15 * mag + np.array([float(r[2]) for r in ref])
    dev = np.hypot(re - wre, im - wim)
    print("dcerror_upper vs hui_w_dw: max |difference| / |w| %.3e" % (dev / mag).max())
    assert np.all(dev <= bar)
    c = mr.hui_coefficients()
    assert c["mwrt_math.hip.h"] == c["mwrt_tl_dev.hip.h"]


def test_planck_b_votes(gpu_ctx):
    x = mr.inputs("planck_bernoulli")[0]
    inv = mh.planck_inv(x)
    n = len(x)
    assert n % 64 != 0
    (part, _, _, _), _ = mh.run(gpu_ctx, "planck_b", (x, inv))
    fullx = np.concatenate([x, np.full(-n % 64, 0.01)])
    (full, _, _, _), _ = mh.run(gpu_ctx, "planck_b", (fullx, mh.planck_inv(fullx)))
    assert np.array_equal(bits(part), bits(full[:n])), "a partial wave took another branch than the full wave of the same values"
    # one lane at 0.05, at 0 or below 0 moves its whole wave to the general branch: every lane still meets that bar, and the
    # waves without such a lane keep their Bernoulli bits
    ref = mh.reference("planck_b_bernoulli")
    for odd in (0.05, 0.0, -0.01):
        y = x.copy()
        y[64 + 13] = odd
        yinv = inv.copy()
        yinv[64 + 13] = 1.0 if odd == 0.0 else 1.0 / odd
        with np.errstate(divide="ignore"):
            (o, _, _, _), _ = mh.run(gpu_ctx, "planck_b", (y, yinv))
        w = np.arange(64, 128)
        w = w[w != 64 + 13]
        assert not np.array_equal(bits(o[w]), bits(part[w])), "the wave stayed on the Bernoulli branch"
        row = mr.check("planck_b wave moved by x = %g" % odd, o[w], [ref[i] for i in w], mh.planck_general_bar(x[w], [ref[i] for i in w]), "general branch")
        assert row["worst_err_over_bar"] <= 1.0
        keep = np.r_[0:64, 128:n]
        assert np.array_equal(bits(o[keep]), bits(part[keep]))


def test_layer_value_flags_and_votes(gpu_ctx):
    x1, x0, live = mr.inputs("layer")
    ref = mh.layer_reference(True)
    negative = np.array([r[0] == "negative" for r in ref])
    out = {}
    for name in ("layer_value_zf1", "layer_value_zf0", "layer_value4", "layer_value_tl_zf1", "layer_value_tl_zf0"):
        out[name], flag = mh.run(gpu_ctx, name, (x1, x0, live))
        if name == "layer_value4":                       # one flag per thread: any of its four elements
            want = np.repeat((negative & (live != 0)).reshape(-1, 4).any(axis=1), 4)
        elif "tl" in name:
            want = negative                               # layer_value_tl has no live argument
        else:
            want = negative & (live != 0)
        assert np.array_equal(flag != 0, want), name
    assert (negative & (live == 0)).any() and (negative & (live != 0)).any()
    # identical lanes with one lane in another band: the wave takes the widest band, every lane within that band's bar
    waves = mh.layer_waves(1)
    assert [w[1] for w in waves[64:70]] == ["mid", "any", "any", "mid", "any", "any"] and all(w[0] == w[1] for w in waves[64:70])
    v = out["layer_value_zf1"][0]
    for w in range(64, 70):
        i = np.arange(64 * w, 64 * w + 64)
        row = mr.check("wave %d" % w, v[i], [ref[k][1] for k in i], np.array([mr.BAR_LV[waves[w][1]] * float(ref[k][1]) for k in i]), "branch of the wave")
        assert row["worst_err_over_bar"] <= 1.0
        same = np.delete(i, 37)
        assert len(set(bits(v[same]))) == 1
    # layer_value4 against four layer_value calls: within the sum of the bars; bit for bit where both waves ran one branch
    v4 = out["layer_value4"][0]
    w4 = mh.layer_waves(4)
    alive = live != 0
    for i in np.flatnonzero(alive):
        b1, b4 = waves[i // 64], w4[i // 256]
        if ref[i][0] in ("negative", "same", "zero"):
            assert bits(v4[i:i + 1])[0] == bits(v[i:i + 1])[0], i
        elif b1[0] == b1[1] == b4[0] == b4[1]:
            assert bits(v4[i:i + 1])[0] == bits(v[i:i + 1])[0], (i, b1, b4)
        else:
            assert abs(v4[i] - v[i]) <= (mr.BAR_LV[b1[1]] + mr.BAR_LV[b4[1]]) * float(ref[i][1]), (i, b1, b4)
    # layer_value_tl: its value within the sum of the bars of layer_value's; its partials exact at the special cases
    for zf, lv in ((True, "layer_value_zf1"), (False, "layer_value_zf0")):
        r = mh.layer_reference(zf)
        t, d1, d0, _ = out["layer_value_tl_zf1" if zf else "layer_value_tl_zf0"]
        bv, _ = mh.tl_bars(x1, x0, r)
        bl = mh._lv_bar(r, waves, 64)
        assert np.all(np.abs(t - out[lv][0])[alive] <= (bv + bl)[alive])
        for k, (br, _, p1, p0) in enumerate(r):
            if br in ("negative", "same", "zero"):
                assert (d1[k], d0[k]) == (float(p1), float(p0)), (k, br)
    kinds = {br: sum(1 for q in ref if q[0] == br) for br in mr.BRANCHES}
    assert all(kinds.values()), kinds


def test_div_small_exhaustive(gpu_ctx):
    n, d = mr.inputs("div_small")
    assert len(n) > 9e5 and d.min() == 1 and d.max() == 1024 and n.max() == 65535
    (o, _, _, _), _ = mh.run(gpu_ctx, "div_small", (n, d))
    want = n.astype(np.int64) // d.astype(np.int64)
    bad = np.flatnonzero(o != want)
    assert len(bad) == 0, (len(bad), n[bad[:5]], d[bad[:5]], o[bad[:5]])


@pytest.mark.parametrize("block", [64, 128, 256, 1024])
def test_block_collectives_are_the_order_emulation(gpu_ctx, block):
    rng = np.random.default_rng(block)
    n = 3 * block - 17                                   # the last workgroup is padded with zeros by the kernel
    v = rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))
    vp = mr.pad(v, block)
    for _ in range(2):                                   # bit-identical between two runs as well
        (s, _, _, _), _ = mh.run(gpu_ctx, "block_sum", (v,), block)
        assert np.array_equal(bits(s), bits(mr.emu_block_sum(vp, block)[:n]))
        (p, t, _, _), _ = mh.run(gpu_ctx, "block_scan", (v,), block)
        ep, et = mr.emu_block_scan(vp, block)
        assert np.array_equal(bits(p), bits(ep[:n])) and np.array_equal(bits(t), bits(et[:n]))
        for g in range(0, n, block):
            assert len(set(bits(t[g:g + block]))) == 1, "block_scan's total differs between lanes"
        (x, _, _, _), _ = mh.run(gpu_ctx, "block_suffix_excl", (v,), block)
        assert np.array_equal(bits(x), bits(mr.emu_block_suffix_excl(vp, block)[:n]))
    # full workgroups: the last lane's suffix is exactly 0
    (x, _, _, _), _ = mh.run(gpu_ctx, "block_suffix_excl", (vp,), block)
    assert np.all(x[block - 1::block] == 0.0) and not np.signbit(x[block - 1::block]).any()


@pytest.mark.parametrize("block", [64, 128, 256, 1024])
def test_block_suffix_keeps_relative_accuracy(gpu_ctx, block):
    """terms falling from 1 to 1e-300 across the workgroup: a total minus a prefix would return 0 (or rounding noise of the
    total) where the true suffix is 1e-300; summed from the top it stays within 64 nthreads eps of the 50-digit sum"""
    v = 10.0 ** np.linspace(0.0, -300.0, block)
    (x, _, _, _), _ = mh.run(gpu_ctx, "block_suffix_excl", (v,), block)
    true = mr.exact_suffix_excl(v, block)
    err = mr.errors(x[:-1], true[:-1])
    rel = err / np.array([float(t) for t in true[:-1]])
    print("block_suffix_excl, %d threads: max relative error %.3e (bar %.3e)" % (block, rel.max(), 64 * block * mr.EPS))
    assert rel.max() <= 64 * block * mr.EPS and x[-1] == 0.0


def test_row16_max(gpu_ctx):
    rng = np.random.default_rng(16)
    v = rng.uniform(0.0, 1.0, 4 * 256).astype(np.float32).astype(np.float64) * 10.0 ** rng.integers(-30, 30, 4 * 256)
    v = v.astype(np.float32).astype(np.float64)
    v[32:48] = 0.0                                       # an all-zero row
    v[48:64] = 0.0
    v[55] = 3.0                                          # a row with a single entry, beside the zero row: no leak
    v[64 + np.arange(16) * 16 + np.arange(16)] = 1e38    # the maximum at each lane position of a row in turn
    (o, _, _, _), _ = mh.run(gpu_ctx, "row16_max", (v,), 256)
    assert np.array_equal(bits(o), bits(mr.emu_row16_max(v)))
    assert np.all(o[32:48] == 0.0) and np.all(o[48:64] == 3.0)


def test_wave_votes_see_active_lanes_only(gpu_ctx):
    n = 3 * 64 + 21                                      # the last wave has 21 active lanes
    p, q = np.ones(n), np.ones(n)
    p[70] = 0.0                                          # wave 1: p fails in one lane
    q[130] = 0.0                                         # wave 2: q fails in one lane
    (al, an, ao, _), _ = mh.run(gpu_ctx, "wave_votes", (p, q), 256)
    w = np.arange(n) // 64
    assert np.array_equal(al, np.where(w == 1, 0.0, 1.0)), "wave_all"
    assert np.all(an == 1.0), "wave_any"
    assert np.array_equal(ao, np.where((w == 1) | (w == 2), 0.0, 1.0)), "wave_all_of: the partial wave must vote true"
    (al, an, ao, _), _ = mh.run(gpu_ctx, "wave_votes", (np.zeros(n), q), 256)
    assert np.all(al == 0.0) and np.all(an == 0.0) and np.all(ao == 0.0)
    z = np.zeros(n)
    z[n - 1] = 1.0                                       # one true lane in the partial wave
    (al, an, ao, _), _ = mh.run(gpu_ctx, "wave_votes", (z, q), 256)
    assert np.array_equal(an, np.where(w == 3, 1.0, 0.0)) and np.all(al == 0.0)


def test_entry_refusals(gpu_ctx):
    x = np.ones(8)
    for kw, helper, said in ((dict(block=100), 0, "multiple of 64"), (dict(block=32), 0, "multiple of 64"), (dict(block=2048), 0, "64..1024"),
                             (dict(block=0), 0, "multiple of 64"), (dict(), len(_native.HELPERS), "unknown helper"), (dict(), -1, "unknown helper"),
                             (dict(n=-1), 0, "n < 0")):
        with pytest.raises(_native.MwrtError) as ei:
            gpu_ctx.selftest_helpers(helper, [] if "n" in kw else [x], **kw)
        assert ei.value.code == -1 and said in str(ei.value), str(ei.value)
    with pytest.raises(_native.MwrtError):
        gpu_ctx.selftest_helpers("layer_value4", [np.ones(6)] * 3)      # n must be a multiple of 4
    outs, flag = gpu_ctx.selftest_helpers("fsqrt", [np.zeros(0)])       # n = 0 is not an error
    assert len(outs[0]) == 0 and len(flag) == 0
