"""The device K-matrix path at its edges, row by row against the exact derivative reference (oracle/tl_oracle.py:
torch autograd of the oracle's formulas on the CPU).

A row is (profile, frequency) over the levels for mwrt_absorption_tl_batch_device and (profile, angle, frequency) over
the levels for mwrt_tb_jacobian_batch_device.  No smoothness mask: the reference follows the device's tangent conventions
 exactly, so every entry is compared; where an absorption tangent differs, the reference's branch
predicate (750-GHz cutoff, speed-dependent switch) must be within 1e-12 relative of its threshold.  Edges: the 64-lane slab and wave seams (nlev 2 ... 1024),
frequency-chunk tails (nf 1 ... 15), every table family and fuzzed tables, dry levels and blocks, identical neighbours,
zero-thickness and 1e-6-km layers, opaque and thin paths, up to 64 angles."""
import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import _native, spectroscopy as sp
from oracle import lbl_oracle as lo
from oracle.fuzz_tables import fuzzed_tables

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
tl = pytest.importorskip("oracle.tl_oracle")

TOL_ROW = 1e-9           # absorption derivatives: of each row's largest |entry|
TOL_VAL = 1e-9           # absorption values and TBs: relative
# K-matrix derivatives: of each row's largest |entry|.  Measured 2.0e-9 at most: where a layer's own
# emission nearly balances the radiance from above it (dTB/dtau_l a difference of two terms ~1e3 times larger, at
# 557 GHz, 4.2 degrees), the kernel's eps * tau_path rounding of its optical-depth prefix sums is amplified by that
# cancellation; 60-digit arithmetic puts the reference within 2.5e-11 there
TOL_K_ROW = 1e-8


def tables(name):
    """(tables, an SD-line frequency inside its speed-dependent window or None)"""
    if name.startswith("fuzz"):
        m, sdl = fuzzed_tables(int(name[4:]))
        return m, float(m.h2o["fl"][sdl[0]]) + 0.3
    m = sp.get_model(name)
    sd = m.h2o["w2"] > 0
    return m, (float(m.h2o["fl"][np.argmax(sd)]) + 0.3 if sd.any() else None)


def frequencies(nf, sd_frq, rot=0):
    """nf frequencies; the first seven are always the edges (in rotation for nf < 7): 2.5, 22.235, 60.3061, 118.7503,
    183.31, 999 GHz and an SD-window point, then a pair straddling the 22-GHz line's 750-GHz cutoff."""
    edge = [60.3061, 22.235, 2.5, 118.7503, 183.31, 999.0, sd_frq if sd_frq else 325.15, 771.9, 772.6]
    rest = [31.4, 51.26, 89.0, 150.0, 325.15, 425.0]
    if nf < len(edge):
        return np.array(np.roll(edge[:7] if nf <= 7 else edge, -rot)[:nf])
    return np.array(edge + rest[:nf - len(edge)])


def profiles(nlev, seed, extreme=False):
    """Three profiles [3][nlev]: moist with dry levels, a dry block and identical neighbours; fully dry; and either a
    second moist one or (extreme=True) the extreme-input generator's 150-340 K, 0.05-1100 hPa, rh 0-1.5.  Heights carry
    repeated levels (dz = 0) and 1e-6-km layers as well as thin and thick ones."""
    rng = np.random.default_rng(seed)
    dz = rng.choice([0.0, 1e-6, 0.005, 0.05, 0.3, 1.5], size=(3, nlev), p=[0.06, 0.06, 0.18, 0.3, 0.3, 0.1])
    dz[:, 0] = 0.0
    if nlev > 3:
        dz[:, min(3, nlev - 1)] = 0.0                       # at least one repeated height and one 1e-6 layer
        dz[:, min(2, nlev - 1)] = 1e-6
    z = np.cumsum(dz, axis=1) + rng.uniform(0.0, 2.0, (3, 1))
    h = z - z[:, :1]
    p = 1013.0 * np.exp(-h / 7.6)
    t = 290.0 - 6.0 * np.minimum(h, 11.0) + rng.normal(0, 0.5, (3, nlev))
    rh = np.clip(0.8 * np.exp(-h / 3.0) + rng.uniform(-0.05, 0.05, (3, nlev)), 0.0, 1.0)
    for i in (0, 2):
        for l in range(4, nlev, 7):                        # identical neighbours (only z differs)
            p[i, l], t[i, l], rh[i, l] = p[i, l - 1], t[i, l - 1], rh[i, l - 1]
        if nlev >= 3:
            rh[i, nlev // 3] = 0.0                          # an isolated dry level
        if nlev >= 12:
            rh[i, nlev // 2: nlev // 2 + 4] = 0.0           # a dry block: moist -> 0, 0 -> 0, 0 -> moist
    rh[1] = 0.0
    if extreme:
        p[2] = np.sort(rng.uniform(0.05, 1100.0, nlev))[::-1]
        t[2] = rng.uniform(150.0, 340.0, nlev)
        rh[2] = rng.uniform(0.0, 1.5, nlev) * (rng.random(nlev) > 0.1)
    return {"z": z, "p": p, "t": t, "rh": rh}


def _dev(P, keys=("z", "p", "t", "rh")):
    return [torch.tensor(np.ascontiguousarray(P[k]), dtype=torch.float64, device="cuda") for k in keys]


def _cur():
    return torch.cuda.current_stream().cuda_stream


def absorption_tl_device(ctx, model, P, frq):
    p, t, rh = _dev(P, ("p", "t", "rh"))
    nprof, nlev = p.shape
    out = [torch.full((nprof, len(frq), nlev), -7.0, dtype=torch.float64, device="cuda") for _ in range(6)]
    ctx.absorption_tl_batch_device(model, nprof, nlev, p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq,
                                   *[o.data_ptr() for o in out], stream=_cur())
    torch.cuda.synchronize()
    return dict(zip(("awet", "adry", "dawet_dt", "dawet_de", "dadry_dt", "dadry_de"), (o.cpu().numpy() for o in out)))


def k_matrix_device(ctx, model, P, frq, ang):
    z, p, t, rh = _dev(P)
    nprof, nlev = z.shape
    opts = dict(dtype=torch.float64, device="cuda")
    tb = torch.full((nprof, len(ang), len(frq)), -7.0, **opts)
    jac = {k: torch.full((nprof, len(ang), len(frq), nlev), -7.0, **opts) for k in ("dtb_dt", "dtb_de", "dtb_ddz")}
    valid = torch.full((nprof,), 9, dtype=torch.uint8, device="cuda")
    ctx.tb_jacobian_batch_device(model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang,
                                 tb.data_ptr(), jac["dtb_dt"].data_ptr(), jac["dtb_de"].data_ptr(),
                                 jac["dtb_ddz"].data_ptr(), valid.data_ptr(), stream=_cur())
    torch.cuda.synchronize()
    return tb.cpu().numpy(), valid.cpu().numpy(), {k: v.cpu().numpy() for k, v in jac.items()}


def row_errors(got, want):
    """|got - want| / (largest |want| of the row), rows over the last axis (0 where the row is all zero and so is got)."""
    scale = np.abs(want).max(axis=-1, keepdims=True)
    err = np.abs(got - want)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))


# ---- mwrt_absorption_tl_batch_device -----------------------------------------------------------------------------
SHAPES = [(1, 2), (6, 63), (7, 64), (8, 65), (14, 129), (15, 1024)]


ABS_MODELS = ["R98", "R17", "R20", "R20SD", "fuzz1", "fuzz2", "fuzz4", "fuzz5"]


def absorption_errors(ctx, name):
    """Largest errors of mwrt_absorption_tl_batch_device against the reference over SHAPES for one table set:
    {"value": relative, "tangent": of the row}.  A tangent entry beyond TOL_ROW must sit where a branch predicate of the
    reference is within 1e-12 relative of its threshold (the kernel may round to the other side); such entries are
    left out of "tangent" and counted in "branch"."""
    m, sdf = tables(name)
    out = {"value": 0.0, "tangent": 0.0, "branch": 0}
    for k, (nf, nlev) in enumerate(SHAPES):
        frq = frequencies(nf, sdf, rot=k)
        P = profiles(nlev, 1000 + 10 * k + len(name), extreme=True)
        got = absorption_tl_device(ctx, m, P, frq)
        for i in range(3):
            e = lo.vapor(P["t"][i], P["rh"][i])[0]
            ref = tl.absorption_tl(m, P["p"][i], P["t"][i], e, frq)
            margin = None
            for key in ("awet", "adry"):
                g, w = got[key][i], ref[key].numpy()
                assert np.isfinite(g).all() and np.isfinite(w).all(), (name, nf, nlev, i, key)
                rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-300 + 1e-13 * np.abs(w).max(axis=-1, keepdims=True))
                out["value"] = max(out["value"], float(rel.max()))
            for key in ("dawet_dt", "dawet_de", "dadry_dt", "dadry_de"):
                rel = row_errors(got[key][i], ref[key].numpy())
                bad = rel > TOL_ROW
                if bad.any():
                    if margin is None:
                        margin = tl.branch_margins(m, P["p"][i], P["t"][i], e, frq)
                    assert (margin[bad] <= 1e-12).all(), (name, nf, nlev, i, key, rel.max())
                    out["branch"] += int(bad.sum())
                out["tangent"] = max(out["tangent"], float(np.where(bad, 0.0, rel).max()))
    return out


@pytest.mark.parametrize("name", ABS_MODELS)
def test_absorption_tl_against_exact_reference(gpu_ctx, name):
    err = absorption_errors(gpu_ctx, name)
    assert err["value"] <= TOL_VAL and err["tangent"] <= TOL_ROW, (name, err)


# ---- mwrt_tb_jacobian_batch_device -------------------------------------------------------------------------------
ANG = np.array([90.0, 30.0, 4.2, 1.0, 179.0])
KCASES = [(2, "R98", 1), (3, "R17", 7), (63, "R20", 8), (64, "R20SD", 15), (65, "fuzz2", 1), (127, "fuzz4", 7),
          (128, "R98", 15), (129, "R20SD", 8), (257, "fuzz2", 15), (1024, "R17", 7)]


def k_row_errors(m, P, frq, ang, tb, valid, jac, profiles_to_check=(0, 1, 2)):
    """Largest errors of a device K-matrix call against the reference: {"TB": relative, "dtb_dt" / "dtb_de" /
    "dtb_ddz": of the row}.  Every entry counts, the levels an opaque path hides included (entries down to 1e-200)."""
    assert (valid == 1).all(), valid
    out = {k: 0.0 for k in ("TB", "dtb_dt", "dtb_de", "dtb_ddz")}
    for i in profiles_to_check:
        ref = tl.k_matrix_rh(m, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], frq, ang)
        rtb = ref["tb"].numpy()
        out["TB"] = max(out["TB"], float((np.abs(tb[i] - rtb) / rtb).max()))
        for key in ("dtb_dt", "dtb_de", "dtb_ddz"):
            out[key] = max(out[key], float(row_errors(jac[key][i], ref[key].numpy()).max()))
    return out


def k_case_errors(ctx, nlev, name, nf):
    m, sdf = tables(name)
    frq = frequencies(nf, sdf)
    P = profiles(nlev, 2000 + nlev)
    tb, valid, jac = k_matrix_device(ctx, m, P, frq, ANG)
    if nf == 1 and nlev > 3:                         # the opaque branch is exercised: 60.3 GHz at 1 degree, tauprof >= TAUMAX
        assert zenith_tau(m, P, 0, frq)[0].sum() / np.sin(np.radians(1.0)) >= lo.TAUMAX
    return k_row_errors(m, P, frq, ANG, tb, valid, jac, profiles_to_check=(0, 1, 2) if nlev <= 257 else (0, 2))


def k_within_tolerance(err):
    return err["TB"] <= TOL_VAL and all(err[k] <= TOL_K_ROW for k in ("dtb_dt", "dtb_de", "dtb_ddz"))


@pytest.mark.parametrize("nlev,name,nf", KCASES, ids=[f"{n}-{m}-nf{f}" for n, m, f in KCASES])
def test_k_matrix_against_exact_reference(gpu_ctx, nlev, name, nf):
    """The workgroup scan on 1-16 waves and the l+1 exchange across every wave seam; one frequency (60.3 GHz: opaque at
    1 degree, no cosmic term), chunk tails; zero and 1e-6-km layers, dry blocks, identical neighbours."""
    err = k_case_errors(gpu_ctx, nlev, name, nf)
    assert k_within_tolerance(err), (nlev, name, nf, err)


def zenith_tau(m, P, i, frq):
    """Layer optical depths at the zenith [nf][nlev] of profile i (the reference's, without grad)."""
    with torch.no_grad():
        e = lo.vapor(P["t"][i], P["rh"][i])[0]
        aw, ad = tl.clearsky_absorption(m, *(torch.tensor(x) for x in (P["p"][i], P["t"][i], e)), frq)
        dz = torch.tensor(np.append(0.0, np.diff(P["z"][i])))
        return (tl.exponential_integration(aw, dz) + tl.exponential_integration(ad, dz)).numpy()


def thin_64_angle_errors(ctx):
    m, sdf = tables("R20SD")
    frq = frequencies(7, sdf)[[0, 1, 2, 3, 4, 6]]
    nlev = 65
    P = profiles(nlev, 77)
    P["z"] = P["z"][:, :1] + np.cumsum(np.full((3, nlev), 0.002), axis=1) - 0.002
    P["z"][:, 10:] -= 0.002                                 # still a zero-thickness layer (layer 10)
    ang = np.linspace(90.0, 2.0, 64)
    assert zenith_tau(m, P, 0, frq).max() <= 0.125
    tb, valid, jac = k_matrix_device(ctx, m, P, frq, ang)
    return k_row_errors(m, P, frq, ang, tb, valid, jac, profiles_to_check=(0,))


def test_k_matrix_thin_layers_and_64_angles(gpu_ctx):
    """One call with 64 elevations (MWRT_MAX_ANGLES) on a profile of thin layers: every layer's tau <= 0.125 at the
    zenith, the small-tau forms of the layer transmittance."""
    err = thin_64_angle_errors(gpu_ctx)
    assert k_within_tolerance(err), err


# ---- zero-thickness layers ---------------------------------------------------------------------------------------
def zero_thickness_case():
    """tests/test_tl_oracle.py's pinned case: a 30-level synthetic R24 profile whose layer 11 has zero thickness."""
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr
    P = pr.synthetic_profiles(1, 0, nlev=30)
    P["z"][0, 11:] -= P["z"][0, 11] - P["z"][0, 10]
    return sp.get_model("R24"), P, np.array([53.86, 22.235, 31.4]), np.array([90.0, 30.0])


def test_zero_thickness_layer_device_and_host(gpu_ctx):
    """dTB/d(thickness) at a zero-thickness layer is g m (Lw + Ld) (9.64 K/km at 53.86 GHz, zenith), not 0: on the device
    K-matrix and on the host entry."""
    m, P, frq, ang = zero_thickness_case()
    ref = tl.k_matrix_rh(m, *(P[k][0] for k in ("z", "p", "t", "rh")), frq, ang)
    assert abs(float(ref["dtb_ddz"][0, 0, 11]) - 9.6415) < 5e-4
    tb, valid, jac = k_matrix_device(gpu_ctx, m, P, frq, ang)
    assert valid.tolist() == [1]
    assert abs(jac["dtb_ddz"][0, 0, 0, 11] - 9.6415) < 5e-4, jac["dtb_ddz"][0, 0, 0, 11]
    for key in ("dtb_dt", "dtb_de", "dtb_ddz"):
        rel = row_errors(jac[key][0], ref[key].numpy())
        assert rel.max() <= TOL_K_ROW, (key, rel.max())
    htb, hvalid, hjac = gpu_ctx.tb_jacobian_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ang)
    assert hvalid.tolist() == [1]
    rel = row_errors(hjac["dtb_ddz"][0], ref["dtb_ddz"].numpy())
    assert rel.max() <= 1e-8, rel.max()


# ---- batch invariance and workspace reuse -----------------------------------------------------------------------
def test_batch_invariance(gpu_ctx):
    """A profile's TBs and rows are bit-identical alone and at positions 0, 17 and 36 of a batch of 37."""
    m, sdf = tables("R20SD")
    frq, ang = frequencies(9, sdf), np.array([90.0, 4.2])
    one = {k: v[:1] for k, v in profiles(129, 5).items()}
    others = profiles(129, 6)
    alone = k_matrix_device(gpu_ctx, m, one, frq, ang)
    for pos in (0, 17, 36):
        big = {k: np.stack([others[k][(i + pos) % 3] for i in range(37)]) for k in one}
        for k in big:
            big[k][pos] = one[k][0]
        tb, valid, jac = k_matrix_device(gpu_ctx, m, big, frq, ang)
        assert np.array_equal(tb[pos], alone[0][0]) and valid[pos] == alone[1][0], pos
        assert all(np.array_equal(jac[k][pos], alone[2][k][0]) for k in jac), pos


def test_workspace_reuse(gpu_ctx):
    """A large call, a small one, the large one again: bit-identical to the same calls on fresh contexts."""
    m = sp.get_model("R24")
    L, S = profiles(180, 8), {k: v[:2, :40] for k, v in profiles(40, 9).items()}
    L = {k: np.tile(v, (40, 1)) for k, v in L.items()}
    fl, al = frequencies(14, None), np.array([90.0, 30.0, 19.2, 14.4, 8.4, 5.4, 4.2])
    fs, as_ = frequencies(3, None), np.array([45.0])
    seq = [k_matrix_device(gpu_ctx, m, X, f, a) for X, f, a in ((L, fl, al), (S, fs, as_), (L, fl, al))]
    for got, (X, f, a) in zip(seq, ((L, fl, al), (S, fs, as_), (L, fl, al))):
        fresh = _native.Context(0)
        try:
            want = k_matrix_device(fresh, m, X, f, a)
        finally:
            fresh.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert all(np.array_equal(got[2][k], want[2][k]) for k in want[2])


# ---- argument validation -----------------------------------------------------------------------------------------
def test_argument_validation_of_the_device_entries(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError
    m = sp.get_model("R24")
    frq, ang = np.array([22.235, 31.4]), np.array([90.0, 30.0])
    opts = dict(dtype=torch.float64, device="cuda")
    # buffers sized for the largest claim below (nlev 1025, 65 angles), so nothing could be written out of bounds
    prof = [torch.ones((2, 1025), **opts) for _ in range(4)]
    big = [torch.full((2 * 65 * 2 * 1025,), -7.0, **opts) for _ in range(6)]
    tb = torch.full((2 * 65 * 2,), -7.0, **opts)
    valid = torch.full((2,), 9, dtype=torch.uint8, device="cuda")
    ptr = [x.data_ptr() for x in prof]

    def absorb(nprof=1, nlev=30, f=frq, null=None):
        outs = [b.data_ptr() for b in big]
        ins = list(ptr[1:])
        if null is not None:
            (ins if null < 3 else outs)[null if null < 3 else null - 3] = 0
        gpu_ctx.absorption_tl_batch_device(m, nprof, nlev, *ins, f, *outs, stream=_cur())

    def kmat(nprof=1, nlev=30, f=frq, a=ang, null=None):
        args = list(ptr) + [tb.data_ptr()] + [b.data_ptr() for b in big[:3]] + [valid.data_ptr()]
        if null is not None:
            args[null] = 0
        gpu_ctx.tb_jacobian_batch_device(m, nprof, nlev, *args[:4], f, a, *args[4:], stream=_cur())

    for call, nnull in ((absorb, 9), (kmat, 9)):
        for k in range(nnull):
            with pytest.raises(MwrtError):
                call(null=k)
        for nlev in (1, 1025):
            with pytest.raises(MwrtError):
                call(nlev=nlev)
        with pytest.raises(MwrtError):
            call(f=np.array([], dtype=np.float64))
        with pytest.raises(MwrtError):
            call(f=np.array([22.235, np.nan]))
    for a in (np.array([], dtype=np.float64), np.full(65, 45.0), np.array([90.0, 0.0]), np.array([180.0])):
        with pytest.raises(MwrtError):
            kmat(a=a)
    torch.cuda.synchronize()
    assert (tb == -7.0).all() and all((b == -7.0).all() for b in big) and (valid == 9).all()
    absorb(nprof=0)                                       # nprof 0: MWRT_OK and nothing written
    kmat(nprof=0)
    torch.cuda.synchronize()
    assert (tb == -7.0).all() and all((b == -7.0).all() for b in big) and (valid == 9).all()


# ---- autograd on the device --------------------------------------------------------------------------------------
def autograd_errors():
    """Largest error of autodiff.brightness_temperature's z, t and rh gradients against the reference's autograd, on the
    zero-thickness case (of the largest entry)."""
    from mwr_fast_forward_operators_and_lbls_amd import autodiff
    m, P, frq, ang = zero_thickness_case()
    z, p, t, rh = _dev(P)
    xs = [x.clone().requires_grad_(True) for x in (z, t, rh)]
    w = np.random.default_rng(3).uniform(-1, 1, (len(ang), len(frq)))
    tb, valid = autodiff.brightness_temperature(m, xs[0], p, xs[1], xs[2], frq, ang)
    (tb[0] * torch.tensor(w, device="cuda")).sum().backward()
    assert valid.cpu().tolist() == [1]
    want = tl.direct_gradients(m, *(P[k][0] for k in ("z", "p", "t", "rh")), frq, ang, weights=w)
    out = {}
    for x, k in zip(xs, ("z", "t", "rh")):
        got, ref = x.grad[0].cpu().numpy(), want[k].numpy()
        out[k] = float(np.abs(got - ref).max() / np.abs(ref).max())
    return out


def test_autograd_on_device_against_exact_reference(gpu_ctx):
    err = autograd_errors()
    assert all(v <= 1e-8 for v in err.values()), err


def test_autograd_nan_profile_and_nan_elevation(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd import autodiff
    m = sp.get_model("R17")
    P = profiles(40, 11)
    P["t"][1, 20] = np.nan
    z, p, t, rh = _dev(P)
    frq = np.array([22.235, 31.4, 52.28])
    xs = [x.clone().requires_grad_(True) for x in (z, t, rh)]
    tb, valid = autodiff.brightness_temperature(m, xs[0], p, xs[1], xs[2], frq, np.array([90.0, 30.0]))
    assert valid.cpu().tolist() == [1, 0, 1]
    tb[[0, 2]].sum().backward()                          # the NaN profile is left out of the loss ...
    for x in xs:
        g = x.grad.cpu().numpy()
        assert np.isnan(g[1]).all() and np.isfinite(g[[0, 2]]).all()     # ... and still gets NaN: NaN in, NaN out
    # a NaN elevation whose TBs are left out of the loss: finite gradients everywhere else
    xs = [x.detach().clone()[[0, 2]].requires_grad_(True) for x in (z, t, rh)]
    tb, valid = autodiff.brightness_temperature(m, xs[0], p[[0, 2]].contiguous(), xs[1], xs[2], frq,
                                                np.array([90.0, np.nan, 30.0]))
    assert valid.cpu().tolist() == [1, 1] and torch.isnan(tb[:, 1]).all()
    tb[:, [0, 2]].sum().backward()
    assert all(torch.isfinite(x.grad).all() for x in xs)
    want = tl.direct_gradients(m, *(P[k][0] for k in ("z", "p", "t", "rh")), frq, np.array([90.0, 30.0]))
    for x, k in zip(xs, ("z", "t", "rh")):
        err = np.abs(x.grad[0].cpu().numpy() - want[k].numpy()).max() / np.abs(want[k].numpy()).max()
        assert err <= 1e-8, (k, err)

