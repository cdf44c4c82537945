"""The device K-matrix along refracted spherical ray paths (mwrt_tb_jacobian_batch_ray_device / mwrt_tb_jacobian_batch_ray,
DESIGN 4.5.4) on the GPU, entry by entry against the exact derivative reference of tests/ray_k_reference.py (torch autograd
through a restatement of the oracle's ray tracer; tests/test_ray_k_reference.py holds it to the oracle and to finite
differences).

Every entry of every row is compared, with no mask: a row is held to ROW_BAR of its largest entry (of its largest sum of
absolute terms where retrieval variables are chained), ROW_BAR = max(TOL_K_ROW, 10 x FLOOR x SHARE) with the conditioning
floor and the path terms' share two constants that tests/test_ray_k_reference.py pins: 1e-8, fixed.  The reference is
evaluated in the device's own (direct-difference) order.  TBs: 1e-9 relative of the reference, 1e-8 K of
mwrt_tb_batch_opt_device(ray_tracing = 1).

Level counts: 2 (one layer: its lower end is the ground), 3, 64 / 65 (the neighbour exchange, the level-0 sum and the
suffix sum across the wave seam), 129, 257 (three and five waves), 1024 (every lane live).  Elevations: both sides of the
zenith branch's edge (90, 89.5), 30, 10.2, 4.2 and 1 degree.  Profiles: tests/test_jacobian_device_edges.profiles, with
zero-thickness and 1e-6-km layers and identical neighbours."""
import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables, MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
rk = pytest.importorskip("ray_k_reference")
kv = pytest.importorskip("kmatrix_variables_reference")

import test_jacobian_device_edges as ed  # noqa: E402
from test_jacobian_cloudy import _cur, _dev, cloudy_profiles  # noqa: E402
from test_jacobian_device_edges import TOL_K_ROW  # noqa: E402
from test_ray_k_reference import FLOOR, SHARE  # noqa: E402

ROW_BAR = max(TOL_K_ROW, 10.0 * FLOOR * SHARE)
TOL_TB_REL = 1e-9          # against the reference
TOL_TB_FWD = 1e-8          # K against mwrt_tb_batch_opt_device(ray_tracing = 1), as the cloudy K entry promises
KEYS = kv.KEYS
ANG = np.array([90.0, 89.5, 30.0, 10.2, 4.2, 1.0])
FRQ3 = np.array([22.24, 31.4, 51.26])
# (nlev, tables, nf)
CASES = [(2, "R98", 1), (3, "R20SD", 7), (64, "fuzz2", 15), (65, "R98", 7), (129, "R20SD", 1), (257, "fuzz2", 7)]


def ray_k_device(ctx, model, P, frq, ang, variables=None, cloud=False, want_ddz=True, fill=-7.0):
    """One mwrt_tb_jacobian_batch_ray_device call -> tb, valid, {the five rows; untouched where not asked for}."""
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    dl = _dev(P["denliq"]) if cloud else None
    di = _dev(P["denice"]) if cloud else None
    nprof, nlev = z.shape
    opts = dict(dtype=torch.float64, device="cuda")
    tb = torch.full((nprof, len(ang), len(frq)), fill, **opts)
    jac = {k: torch.full((nprof, len(ang), len(frq), nlev), fill, **opts) for k in KEYS}
    valid = torch.full((nprof,), 9, dtype=torch.uint8, device="cuda")
    if isinstance(variables, tuple):
        variables = JacVariables(*variables, 0)
    ptr = lambda k, on=True: jac[k].data_ptr() if on else None   # noqa: E731
    ctx.tb_jacobian_batch_ray_device(
        model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb.data_ptr(),
        ptr("dtb_dt"), ptr("dtb_dh"), valid.data_ptr(), d_dtb_ddz=ptr("dtb_ddz", want_ddz),
        d_denliq=None if dl is None else dl.data_ptr(), d_denice=None if di is None else di.data_ptr(),
        d_dtb_dliq=ptr("dtb_dliq", cloud), d_dtb_dice=ptr("dtb_dice", cloud), variables=variables, stream=_cur())
    torch.cuda.synchronize()
    return tb, valid, jac


def forward_ray(ctx, model, P, frq, ang, cloud=False):
    """mwrt_tb_batch_opt_device(ray_tracing = 1) -> tb, valid (NumPy)."""
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    nprof, nlev = z.shape
    tb = torch.full((nprof, len(ang), len(frq)), -7.0, dtype=torch.float64, device="cuda")
    valid = torch.full((nprof,), 9, dtype=torch.uint8, device="cuda")
    den = [_dev(P["denliq"]), _dev(P["denice"])] if cloud else []       # (kept alive until the call has run)
    kw = dict(d_denliq=den[0].data_ptr(), d_denice=den[1].data_ptr()) if cloud else {}
    ctx.tb_batch_device(model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb.data_ptr(),
                        valid.data_ptr(), stream=_cur(), ray_tracing=True, **kw)
    torch.cuda.synchronize()
    return tb.cpu().numpy(), valid.cpu().numpy()


def _np(x):
    return x.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(_np(a) if isinstance(a, torch.Tensor) else a, _np(b) if isinstance(b, torch.Tensor) else b,
                          equal_nan=True)


@pytest.mark.parametrize("nlev,name,nf", CASES, ids=[f"{c[0]}-{c[1]}-nf{c[2]}" for c in CASES])
def test_rows_and_tb_against_the_reference(gpu_ctx, nlev, name, nf):
    m, sdf = ed.tables(name)
    frq = ed.frequencies(nf, sdf, rot=nlev % 7)
    P = ed.profiles(nlev, 4200 + nlev)
    tb, valid, jac = ray_k_device(gpu_ctx, m, P, frq, ANG)
    tb, valid = _np(tb), _np(valid)
    ftb, fvalid = forward_ray(gpu_ctx, m, P, frq, ANG)
    assert np.array_equal(valid, fvalid) and np.array_equal(np.isnan(tb), np.isnan(ftb)), (valid, fvalid)
    err = {k: 0.0 for k in ("TB", "TB_fwd", "dtb_dt", "dtb_dh", "dtb_ddz")}
    err["TB_fwd"] = float(np.nanmax(np.abs(tb - ftb)))
    for i in range(3):
        args = [P[k][i] for k in ("z", "p", "t", "rh")]
        # the device forms a layer's angles directly, not from running sums: the reference is asked for that order
        K = {k: v.detach().numpy() for k, v in rk.k_matrix_ray_rh(m, *args, frq, ANG, order="direct").items()}
        trapped = np.isnan(K["tb"]).any(axis=1)
        assert valid[i] == (3 if trapped.any() else 1), (i, valid[i], trapped)
        ok = ~trapped
        assert np.isnan(tb[i, trapped]).all() and np.isfinite(tb[i, ok]).all()
        err["TB"] = max(err["TB"], float((np.abs(tb[i, ok] - K["tb"][ok]) / K["tb"][ok]).max()))
        for k, rk_key in (("dtb_dt", "dtb_dt"), ("dtb_dh", "dtb_de"), ("dtb_ddz", "dtb_ddz")):
            got = _np(jac[k])[i]
            assert np.isnan(got[trapped]).all() and np.isfinite(got[ok]).all(), (i, k)
            err[k] = max(err[k], float(ed.row_errors(got[ok], K[rk_key][ok]).max()))
        assert (_np(jac["dtb_ddz"])[i, ok, :, 0] == 0.0).all()             # the ground has no layer below it
    assert (jac["dtb_dliq"] == -7.0).all() and (jac["dtb_dice"] == -7.0).all()      # not asked for: not written
    print(nlev, name, nf, err, "row bar", ROW_BAR)
    assert err["TB"] <= TOL_TB_REL and err["TB_fwd"] <= TOL_TB_FWD, err
    assert all(err[k] <= ROW_BAR for k in ("dtb_dt", "dtb_dh", "dtb_ddz")), (err, ROW_BAR)


_cloud_ref = {}


def cloud_reference():
    """(tables, profiles, [raw reference K per profile]) at 65 levels with liquid and ice, computed once."""
    if not _cloud_ref:
        m = sp.get_model("R24")
        P = cloudy_profiles(65, 3, 365)
        K = [{k: v.detach().numpy() for k, v in rk.k_matrix_ray_rh(
            m, *(P[k][i] for k in ("z", "p", "t", "rh")), FRQ3, ANG, denliq=P["denliq"][i], denice=P["denice"][i]).items()}
            for i in range(3)]
        _cloud_ref["ref"] = (m, P, K)
    return _cloud_ref["ref"]


@pytest.mark.parametrize("variables", [(0, 0, 0), (1, 0, 1), (2, 1, 1)])
def test_variables_and_cloud_against_the_chained_reference(gpu_ctx, variables):
    m, P, K = cloud_reference()
    tb, valid, jac = ray_k_device(gpu_ctx, m, P, FRQ3, ANG, variables, cloud=True)
    assert valid.cpu().tolist() == [1, 1, 1]
    ftb, _ = forward_ray(gpu_ctx, m, P, FRQ3, ANG, cloud=True)
    err = {k: 0.0 for k in ("TB", "TB_fwd") + KEYS}
    err["TB_fwd"] = float(np.abs(_np(tb) - ftb).max())
    for i in range(3):
        want, scale = kv.chain(K[i], P["p"][i], P["t"][i], P["rh"][i], P["denliq"][i], P["denice"][i], variables)
        err["TB"] = max(err["TB"], float((np.abs(_np(tb)[i] - K[i]["tb"]) / K[i]["tb"]).max()))
        for k in KEYS:
            err[k] = max(err[k], float(kv.scaled_row_errors(_np(jac[k])[i], want[k], scale[k]).max()))
    assert np.abs(K[0]["dtb_dliq"]).max() > 1.0 and np.abs(K[0]["dtb_dice"]).max() > 1e-2       # the cloud is there
    print(variables, err)
    assert err["TB"] <= TOL_TB_REL and err["TB_fwd"] <= TOL_TB_FWD, err
    assert all(err[k] <= ROW_BAR for k in KEYS), err


def test_null_variables_equal_all_zero_variables_bit_for_bit(gpu_ctx):
    m, P, _ = cloud_reference()
    for cloud in (True, False):
        a = ray_k_device(gpu_ctx, m, P, FRQ3, ANG, None, cloud=cloud)
        b = ray_k_device(gpu_ctx, m, P, FRQ3, ANG, (0, 0, 0), cloud=cloud)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and all(same_bits(a[2][k], b[2][k]) for k in KEYS)
        c = ray_k_device(gpu_ctx, m, P, FRQ3, ANG, None, cloud=cloud, want_ddz=False)
        assert (c[2]["dtb_ddz"] == -7.0).all() and all(same_bits(a[2][k], c[2][k]) for k in KEYS if k != "dtb_ddz")


def ducting_profiles(nlev=33):
    """Three profiles, the middle one with a surface duct: saturated at the ground, rh <= 0.05 above, and an 8-K inversion
    in the first, 100-m layer -- 0.5 degrees is trapped, 4.2 degrees is not."""
    P = ed.profiles(nlev, 99)
    h = np.concatenate([[0.0, 0.1], np.linspace(0.4, 12.0, nlev - 2)])      # a 100-m surface layer
    P["z"][1] = 0.1 + h
    P["p"][1] = 1013.0 * np.exp(-h / 7.6)
    P["t"][1] = 288.0 - 6.0 * h
    P["t"][1, 1] = P["t"][1, 0] + 8.0
    P["rh"][1] = 0.05
    P["rh"][1, 0] = 1.0
    return P


def test_trapped_ray_is_flag_three_and_blanks_its_elevation_only(gpu_ctx):
    m = sp.get_model("R24")
    P = ducting_profiles()
    ang = np.array([90.0, 4.2, 0.5])
    tb, valid, jac = ray_k_device(gpu_ctx, m, P, FRQ3, ang)
    ftb, fvalid = forward_ray(gpu_ctx, m, P, FRQ3, ang)
    assert valid.cpu().tolist() == fvalid.tolist() and valid[1] == 3, (valid, fvalid)
    assert np.array_equal(np.isnan(_np(tb)), np.isnan(ftb))
    assert torch.isnan(tb[1, 2]).all() and all(torch.isnan(jac[k][1, 2]).all() for k in KEYS[:3])
    tb2, valid2, jac2 = ray_k_device(gpu_ctx, m, P, FRQ3, ang[:2])
    assert valid2[1] == 1
    assert same_bits(tb[:, :2], tb2) and all(same_bits(jac[k][:, :2], jac2[k]) for k in KEYS[:3])
    for i in (0, 2):                                          # the batch-mates are untouched, whatever their own flag is
        assert valid[i] == fvalid[i]
        if valid[i] == 1:
            assert torch.isfinite(tb[i]).all()


def test_nan_handling(gpu_ctx):
    m, P, _ = cloud_reference()
    ang = np.array([90.0, np.nan, 4.2])
    want = ray_k_device(gpu_ctx, m, P, FRQ3, ang, (1, 0, 0), cloud=True)
    assert want[1].cpu().tolist() == [1, 1, 1]
    assert torch.isnan(want[0][:, 1]).all() and all(torch.isnan(want[2][k][:, 1]).all() for k in KEYS)
    assert torch.isfinite(want[0][:, [0, 2]]).all() and all(torch.isfinite(want[2][k][:, [0, 2]]).all() for k in KEYS)
    for key in ("z", "p", "t", "rh", "denliq", "denice"):             # a NaN in the profile: valid 0, every row of the profile NaN
        Q = {k: v.copy() for k, v in P.items()}
        Q[key][1, 64] = np.nan
        tb, valid, jac = ray_k_device(gpu_ctx, m, Q, FRQ3, ang, (1, 0, 0), cloud=True)
        assert valid.cpu().tolist() == [1, 0, 1], key
        assert torch.isnan(tb[1]).all() and all(torch.isnan(jac[k][1]).all() for k in KEYS), key
        for i in (0, 2):
            assert same_bits(tb[i], want[0][i]) and all(same_bits(jac[k][i], want[2][k][i]) for k in KEYS), (key, i)
        ftb, fvalid = forward_ray(gpu_ctx, m, Q, FRQ3, ang, cloud=True)
        assert fvalid.tolist() == [1, 0, 1] and np.array_equal(np.isnan(ftb), np.isnan(_np(tb))), key


def test_every_lane_live_and_batch_independence(gpu_ctx):
    """1024 levels, one frequency, two elevations: finite rows, the forward entry's TBs, and a profile's outputs bit-identical
    in a batch of one and a batch of five."""
    m = sp.get_model("R98")
    frq, ang = np.array([31.4]), np.array([30.0, 4.2])
    E = ed.profiles(1024, 5)
    P = {k: np.concatenate([v, v[:2]]) for k, v in E.items()}          # five profiles
    tb, valid, jac = ray_k_device(gpu_ctx, m, P, frq, ang)
    ftb, fvalid = forward_ray(gpu_ctx, m, P, frq, ang)
    assert valid.cpu().tolist() == fvalid.tolist() == [1] * 5
    assert torch.isfinite(tb).all() and all(torch.isfinite(jac[k]).all() for k in KEYS[:3])
    assert np.abs(_np(tb) - ftb).max() <= TOL_TB_FWD
    one = ray_k_device(gpu_ctx, m, {k: v[2:3] for k, v in P.items()}, frq, ang)
    assert same_bits(one[0], tb[2:3]) and all(same_bits(one[2][k], jac[k][2:3]) for k in KEYS[:3])


def test_host_entry_equals_device_entry_and_frees_its_staging(gpu_ctx):
    m, P, _ = cloud_reference()
    ang = np.array([90.0, np.nan, 4.2])
    variables = JacVariables(1, 1, 1, 0)
    tb, valid, jac = ray_k_device(gpu_ctx, m, P, FRQ3, ang, variables, cloud=True)
    args = [P[k] for k in ("z", "p", "t", "rh")]

    def host(v, **kw):
        return gpu_ctx.tb_jacobian_batch_ray(m, *args, FRQ3, ang, denliq=P["denliq"], denice=P["denice"], variables=v, **kw)
    htb, hvalid, hjac = host(variables)
    assert same_bits(htb, tb) and same_bits(hvalid, valid) and sorted(hjac) == sorted(KEYS)
    assert all(same_bits(hjac[k], jac[k]) for k in KEYS)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(MwrtError) as ei:
        host(JacVariables(0, 0, 5, 0))
    assert ei.value.code == -1
    assert torch.cuda.mem_get_info()[0] == free0
    host(variables)
    assert torch.cuda.mem_get_info()[0] == free0


def test_repeat_call_allocates_nothing_and_repeats_its_bits(gpu_ctx):
    m = sp.get_model("R24")
    for nlev in (180, 385):
        P = cloudy_profiles(nlev, 4, 61)
        ray_k_device(gpu_ctx, m, P, FRQ3, ANG, (2, 1, 1), cloud=True)          # warm-up: the workspaces grow here
        torch.cuda.synchronize()
        arrs = {k: _dev(P[k]) for k in P}
        opts = dict(dtype=torch.float64, device="cuda")
        tb = torch.empty((4, len(ANG), 3), **opts)
        jac = [torch.empty((4, len(ANG), 3, nlev), **opts) for _ in range(4)]
        valid = torch.empty(4, dtype=torch.uint8, device="cuda")

        def call():
            gpu_ctx.tb_jacobian_batch_ray_device(
                m, 4, nlev, *(arrs[k].data_ptr() for k in ("z", "p", "t", "rh")), FRQ3, ANG, tb.data_ptr(), jac[0].data_ptr(),
                jac[1].data_ptr(), valid.data_ptr(), d_denliq=arrs["denliq"].data_ptr(), d_denice=arrs["denice"].data_ptr(),
                d_dtb_dliq=jac[2].data_ptr(), d_dtb_dice=jac[3].data_ptr(), variables=JacVariables(2, 1, 1, 0), stream=_cur())
            torch.cuda.synchronize()
        call()
        first = [j.clone() for j in jac] + [tb.clone()]
        free0 = torch.cuda.mem_get_info()[0]
        call()
        assert torch.cuda.mem_get_info()[0] == free0, nlev
        assert all(torch.equal(a, b) for a, b in zip(first, jac + [tb]))


def test_refusals_write_nothing(gpu_ctx):
    m, P, _ = cloud_reference()
    z, p, t, rh, dl = (_dev(P[k]) for k in ("z", "p", "t", "rh", "denliq"))
    opts = dict(dtype=torch.float64, device="cuda")
    out = [torch.full((3, 2, 3, 65), -7.0, **opts) for _ in range(5)]
    tb = torch.full((3, 2, 3), -7.0, **opts)
    valid = torch.full((3,), 9, dtype=torch.uint8, device="cuda")
    ang = np.array([90.0, 4.2])

    def call(nlev=65, frq=FRQ3, ang=ang, null=None, **kw):
        a = dict(d_z=z.data_ptr(), d_p=p.data_ptr(), d_t=t.data_ptr(), d_rh=rh.data_ptr(), d_tb=tb.data_ptr(),
                 d_dtb_dt=out[0].data_ptr(), d_dtb_dh=out[1].data_ptr(), d_valid=valid.data_ptr())
        if null:
            a[null] = 0
        gpu_ctx.tb_jacobian_batch_ray_device(m, 3, nlev, a["d_z"], a["d_p"], a["d_t"], a["d_rh"], frq, ang, a["d_tb"],
                                             a["d_dtb_dt"], a["d_dtb_dh"], a["d_valid"], d_dtb_ddz=out[2].data_ptr(),
                                             stream=_cur(), **kw)
    cases = [(dict(null=k), -1) for k in ("d_z", "d_p", "d_t", "d_rh", "d_tb", "d_dtb_dt", "d_dtb_dh", "d_valid")]
    cases += [(dict(nlev=1), -1), (dict(frq=np.array([])), -1), (dict(frq=np.array([22.24, np.nan])), -1),
              (dict(ang=np.linspace(5.0, 85.0, 65)), -1), (dict(variables=JacVariables(3, 0, 0, 0)), -1),
              (dict(variables=JacVariables(0, 0, 0, 7)), -1), (dict(d_dtb_dliq=out[3].data_ptr()), -1),
              (dict(d_dtb_dice=out[4].data_ptr()), -1)]
    for kw, code in cases:
        with pytest.raises(MwrtError) as ei:
            call(**kw)
        assert ei.value.code == code, kw
    # one lane per level: 1025 levels get the status the vars entry gives them (MWRT_ERR_UNSUPPORTED from the shared check)
    with pytest.raises(MwrtError) as ei:
        call(nlev=1025)
    assert ei.value.code == -5
    with pytest.raises(MwrtError) as ei:                    # no ozone tangent
        gpu_ctx._jacobian_vars_device("mwrt_tb_jacobian_batch_ray_device", m, 3, 65, z.data_ptr(), p.data_ptr(), t.data_ptr(),
                                      rh.data_ptr(), FRQ3, ang, tb.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                      valid.data_ptr(), None, _options_with_o3n(dl), None, None, None, _cur())
    assert ei.value.code == -5
    torch.cuda.synchronize()
    assert (tb == -7.0).all() and all((o == -7.0).all() for o in out) and (valid == 9).all()


def _options_with_o3n(d):
    from mwr_fast_forward_operators_and_lbls_amd import _native
    return _native._options(None, None, False, d.data_ptr())


def test_one_d_var_step_is_better_with_rays_on_ray_made_observations(gpu_ctx):
    """8 profiles, 33 levels, 4 frequencies, elevations down to 4.2 degrees; y = the ray-traced forward operator at x_true,
    xa = x_true, x = x_true + 0.2 sigma (a smooth bump).  One step with ray_tracing=True and one without: without rays
    y - F(x_true) is the multi-kelvin geometry bias, with rays it is second order in the bump."""
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    nprof, nlev = 8, 33
    frq, elev = np.array([22.24, 31.4, 51.26, 58.0]), np.array([90.0, 30.0, 10.2, 4.2])
    rng = np.random.default_rng(12)
    h = np.linspace(0.0, 14.0, nlev) ** 1.0
    z = np.tile(0.2 + h, (nprof, 1))
    p = np.tile(1010.0 * np.exp(-h / 7.7), (nprof, 1))
    t_true = 288.0 + rng.normal(0.0, 2.0, (nprof, 1)) - 6.2 * np.minimum(h, 11.5)[None]
    rh_true = np.clip(0.75 * np.exp(-h / 3.0)[None] + rng.uniform(-0.05, 0.05, (nprof, 1)), 0.02, 0.95)
    sig = np.array([1.5, 0.08])
    lev = np.arange(nlev)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 4.0)
    sa = np.zeros((2 * nlev, 2 * nlev))
    for b in range(2):
        sa[b * nlev:(b + 1) * nlev, b * nlev:(b + 1) * nlev] = sig[b] ** 2 * corr
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    x_true = dev(np.stack([t_true, rh_true], axis=1))
    bump = np.exp(-0.5 * ((h - 2.0) / 1.5) ** 2)
    x0 = x_true + 0.2 * dev(sig[None, :, None] * bump[None, None, :])
    zt, pt = dev(z), dev(p)
    m = sp.get_model("R24")
    P = dict(z=z, p=p, t=t_true, rh=rh_true)
    y_np, v = forward_ray(gpu_ctx, m, P, frq, elev)
    assert (v == 1).all()
    y = dev(y_np)
    moved = {}
    for rays in (True, False):
        ov = retrieval.OneDVar(m, frq, elev, dev(sa), dev(np.full(frq.size * elev.size, 0.25)),
                               variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=x_true, ray_tracing=rays)
        x_new, d = ov.step(zt, pt, x0, y)
        assert ((d["status"] == 1) | (d["status"] == 3)).all(), d["status"]
        moved[rays] = ((x_new - x_true).abs() / dev(sig)[None, :, None]).amax(dim=(1, 2)).cpu().numpy()
        if rays:
            ftb, fv = ov.forward(zt, pt, x_true)
            assert (fv == 1).all() and np.abs(_np(ftb) - y_np).max() <= TOL_TB_FWD
    print("max |x+ - x_true| / sigma per profile, ray step:", moved[True], "flat step:", moved[False])
    assert (moved[True] < moved[False]).all(), moved
