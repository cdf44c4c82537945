"""The device K-matrix in retrieval variables (mwrt_tb_jacobian_batch_vars_device / mwrt_tb_jacobian_batch_vars, DESIGN
4.5.3) on the GPU, entry by entry against ``chain(reference K)``: the header's chain-rule formulas
(tests/kmatrix_variables_reference.py, held to end-to-end autograd by tests/test_kmatrix_variables_cpu.py) applied to the
exact derivative reference of tests/cloudy_tl_reference.py.

Every entry of every row is compared in all 12 combinations of humidity x cloud x heights, with no mask and no floor.
Tolerance per row: TOL_K_ROW (1e-8) of the row's largest sum of absolute terms from the reference -- each raw row is held
to 1e-8 of its own scale already, and a chained entry is a sum of at most five such terms times exact factors.  A
reference row whose terms are all zero must be exactly zero on the device.

Level counts: 2 (one layer: level 0 has c = 0 and the top has no upper neighbour), 3 (one interior level), 64 / 65 (the
s2[tid + 1] exchange across the wave seam), 180 (the workload's), 1024 (every lane live, the largest LDS), and the two
sides of the 64-KiB dynamic-LDS opt-in of a launch with a mode set.  Such a launch holds 3 + 9 = 12 LDS rows of one double
per lane clear and 3 + 7 + 9 = 19 cloudy (+ 16 doubles), lanes = levels rounded up to 64: 12 x 640 x 8 + 128 = 61 568 B at
640 levels and 67 712 B from 641 on; 19 x 384 x 8 + 128 = 58 496 B at 384 and 68 224 B from 385 on."""
import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables, MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
cr = pytest.importorskip("cloudy_tl_reference")
kv = pytest.importorskip("kmatrix_variables_reference")

from test_jacobian_device_edges import TOL_K_ROW, TOL_VAL  # noqa: E402
from test_jacobian_cloudy import ANG, FRQ, GOOD, _cur, _dev, cloudy_k_device, cloudy_profiles  # noqa: E402

KEYS = kv.KEYS
# (nlev, model, nf, profiles, cloud arrays passed): R98 is liq_mode 0, R24 liq_mode 1
CASES = [(2, "R98", 1, 3, True), (3, "R24", 2, 3, True), (64, "R24", 2, 3, True), (65, "R98", 3, 3, True),
         (180, "R24", 3, 3, True), (384, "R98", 1, 2, True), (385, "R24", 1, 2, True), (640, "R24", 1, 2, False),
         (641, "R98", 1, 2, False), (1024, "R24", 2, 2, True)]


def vars_k_device(ctx, model, P, frq, ang, variables, cloud=True, want_ddz=True, fill=-7.0, **kw):
    """One mwrt_tb_jacobian_batch_vars_device call -> tb, valid, {the five rows; None where not asked for}.  variables: a
    (humidity, cloud, heights) tuple, a JacVariables, or None (NULL)."""
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
    ctx.tb_jacobian_batch_vars_device(
        model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, tb.data_ptr(),
        ptr("dtb_dt"), ptr("dtb_dh"), valid.data_ptr(), d_dtb_ddz=ptr("dtb_ddz", want_ddz),
        d_denliq=None if dl is None else dl.data_ptr(), d_denice=None if di is None else di.data_ptr(),
        d_dtb_dliq=ptr("dtb_dliq", cloud), d_dtb_dice=ptr("dtb_dice", cloud), variables=variables, stream=_cur(), **kw)
    torch.cuda.synchronize()
    return tb, valid, jac


def _np(x):
    return x.cpu().numpy()


_refs = {}


def reference(name, nlev, nf, nprof, cloud):
    """(model, profiles, frequencies, [raw reference K-matrix per profile]) of a case, computed once."""
    key = (name, nlev, nf, nprof, cloud)
    if key not in _refs:
        m = sp.get_model(name)
        frq = FRQ[:nf] if nf > 1 else FRQ[1:2]
        P = cloudy_profiles(nlev, nprof, 300 + nlev)
        K = []
        for i in range(nprof):
            args = [P[k][i] for k in ("z", "p", "t", "rh")] + [P[k][i] if cloud else None for k in ("denliq", "denice")]
            K.append({k: v.detach().numpy() for k, v in cr.k_matrix_cloudy_rh(m, *args, frq, ANG[GOOD]).items()})
        _refs[key] = (m, P, frq, K)
    return _refs[key]


def case_errors(ctx, nlev, name, nf, nprof, cloud):
    """Largest error of each row kind over all 12 mode combinations, of the row's largest sum of absolute terms
    ("TB": relative)."""
    m, P, frq, K = reference(name, nlev, nf, nprof, cloud)
    out = {k: 0.0 for k in ("TB",) + KEYS}
    keys = KEYS if cloud else KEYS[:3]
    for variables in kv.ALL_VARIABLES:
        tb, valid, jac = vars_k_device(ctx, m, P, frq, ANG, variables, cloud=cloud)
        assert valid.cpu().tolist() == [1] * nprof, (variables, valid)
        tb, jac = _np(tb), {k: _np(jac[k]) for k in keys}
        # the NaN elevation blanks its own rows only
        assert np.isnan(tb[:, ~GOOD]).all() and all(np.isnan(jac[k][:, ~GOOD]).all() for k in keys)
        for i in range(nprof):
            want, scale = kv.chain(K[i], P["p"][i], P["t"][i], P["rh"][i], P["denliq"][i], P["denice"][i], variables)
            out["TB"] = max(out["TB"], float((np.abs(tb[i, GOOD] - K[i]["tb"]) / K[i]["tb"]).max()))
            for k in keys:
                out[k] = max(out[k], float(kv.scaled_row_errors(jac[k][i, GOOD], want[k], scale[k]).max()))
    if cloud and 3 < nlev <= 180:                          # the cloud is there: rows of K per g m-3, not rounding
        assert np.abs(K[0]["dtb_dliq"]).max() > 1.0 and np.abs(K[0]["dtb_dice"]).max() > 1e-2
    return out


@pytest.mark.parametrize("nlev,name,nf,nprof,cloud", CASES, ids=[f"{c[0]}-{c[1]}-nf{c[2]}-{'cloudy' if c[4] else 'clear'}" for c in CASES])
def test_every_mode_combination_against_the_chained_reference(gpu_ctx, nlev, name, nf, nprof, cloud):
    err = case_errors(gpu_ctx, nlev, name, nf, nprof, cloud)
    print(nlev, name, nf, err)
    assert err["TB"] <= TOL_VAL, err
    assert all(err[k] <= TOL_K_ROW for k in KEYS), err


@pytest.mark.parametrize("nlev,name", [(65, "R98"), (180, "R24")])
def test_null_and_zero_variables_are_the_opt_entry_bit_for_bit(gpu_ctx, nlev, name):
    """vars NULL and vars all zero: every output torch.equal to mwrt_tb_jacobian_batch_opt_device's, clear and cloudy;
    d_dtb_ddz = NULL leaves the other rows bit-identical and writes no thickness row."""
    m = sp.get_model(name)
    P = cloudy_profiles(nlev, 4, 7)
    ang = ANG[GOOD]
    for cloud in (True, False):
        tb0, v0, j0 = cloudy_k_device(gpu_ctx, m, P, FRQ, ang, liq=cloud, ice=cloud)
        j0["dtb_dh"] = j0.pop("dtb_de")
        for variables in (None, (0, 0, 0)):
            for want_ddz in (True, False):
                tb, v, j = vars_k_device(gpu_ctx, m, P, FRQ, ang, variables, cloud=cloud, want_ddz=want_ddz)
                assert torch.equal(tb.cpu(), torch.tensor(tb0)) and torch.equal(v.cpu(), torch.tensor(v0))
                for k in KEYS:
                    if k == "dtb_ddz" and not want_ddz or (not cloud and k in KEYS[3:]):
                        assert (j[k] == -7.0).all(), k        # not asked for: not written
                    else:
                        assert torch.equal(j[k].cpu(), torch.tensor(j0[k])), (k, variables, want_ddz, cloud)


def test_thickness_row_is_raw_and_optional_in_every_mode(gpu_ctx):
    """Given, d_dtb_ddz is the raw thickness row whatever the modes; left out, the other rows do not change."""
    m = sp.get_model("R24")
    P = cloudy_profiles(65, 3, 17)
    ang = ANG[GOOD][:2]
    raw = vars_k_device(gpu_ctx, m, P, FRQ, ang, None)[2]["dtb_ddz"]
    for variables in ((2, 1, 1), (1, 0, 1), (0, 1, 0)):
        _, _, full = vars_k_device(gpu_ctx, m, P, FRQ, ang, variables)
        _, _, bare = vars_k_device(gpu_ctx, m, P, FRQ, ang, variables, want_ddz=False)
        assert torch.equal(full["dtb_ddz"], raw) and (bare["dtb_ddz"] == -7.0).all()
        assert all(torch.equal(full[k], bare[k]) for k in KEYS if k != "dtb_ddz")


def test_nan_inputs_and_refusals(gpu_ctx):
    m = sp.get_model("R24")
    P = cloudy_profiles(65, 3, 41)
    ang = np.array([90.0, np.nan, 4.2])
    want = vars_k_device(gpu_ctx, m, P, FRQ, ang, (2, 1, 1))
    assert want[1].cpu().tolist() == [1, 1, 1]
    for key in ("p", "t"):                                   # a NaN in p or T: valid 0, every row of the profile NaN
        Q = {k: v.copy() for k, v in P.items()}
        Q[key][1, 64] = np.nan
        tb, valid, jac = vars_k_device(gpu_ctx, m, Q, FRQ, ang, (2, 1, 1))
        assert valid.cpu().tolist() == [1, 0, 1], key
        assert torch.isnan(tb[1]).all() and all(torch.isnan(jac[k][1]).all() for k in KEYS)
        for i in (0, 2):                                     # the neighbours are untouched, the NaN elevation blanks its own rows
            assert torch.equal(tb[i, [0, 2]], want[0][i, [0, 2]]) and torch.isnan(tb[i, 1]).all()
            assert all(torch.equal(jac[k][i, [0, 2]], want[2][k][i, [0, 2]]) and torch.isnan(jac[k][i, 1]).all() for k in KEYS)
    # refusals: nothing is written
    bad = [(JacVariables(3, 0, 0, 0), {}, -1), (JacVariables(-1, 0, 0, 0), {}, -1), (JacVariables(0, 2, 0, 0), {}, -1),
           (JacVariables(0, 0, 2, 0), {}, -1), (JacVariables(0, 0, -1, 0), {}, -1), (JacVariables(2, 1, 1, 1), {}, -1),
           ((2, 1, 1), dict(ray_tracing=True), -5)]
    for variables, kw, code in bad:
        with pytest.raises(MwrtError) as ei:
            vars_k_device(gpu_ctx, m, P, FRQ, ang, variables, **kw)
        assert ei.value.code == code, (variables, kw)
    z, p, t, rh, dl = (_dev(P[k]) for k in ("z", "p", "t", "rh", "denliq"))
    out = [torch.full((3, 3, 3, 65), -7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    tb = torch.full((3, 3, 3), -7.0, dtype=torch.float64, device="cuda")
    valid = torch.full((3,), 9, dtype=torch.uint8, device="cuda")
    for kw, code in ((dict(d_o3n=dl.data_ptr()), -5), (dict(variables=JacVariables(0, 0, 0, 7)), -1)):
        with pytest.raises(MwrtError) as ei:
            gpu_ctx.tb_jacobian_batch_vars_device(m, 3, 65, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), FRQ, ang,
                                                  tb.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), valid.data_ptr(),
                                                  stream=_cur(), **kw)
        assert ei.value.code == code, kw
    torch.cuda.synchronize()
    assert (tb == -7.0).all() and all((o == -7.0).all() for o in out) and (valid == 9).all()


def test_host_entry_equals_device_entry_and_frees_its_staging(gpu_ctx):
    """mwrt_tb_jacobian_batch_vars on NumPy arrays: bit for bit the device entry (65 levels, cloudy, a NaN elevation and
    a NaN profile included); a refusal that arrives after staging has begun -- the device entry it calls makes the checks
    -- leaves the free device memory where it was, and so does a successful call."""
    m = sp.get_model("R98")
    P = cloudy_profiles(65, 4, 27)
    P["t"][3, 10] = np.nan
    ang = np.array([90.0, np.nan, 4.2])
    variables = JacVariables(1, 1, 1, 0)
    tb, valid, jac = vars_k_device(gpu_ctx, m, P, FRQ, ang, variables)
    assert valid.cpu().tolist() == [1, 1, 1, 0]
    args = [P[k] for k in ("z", "p", "t", "rh")]

    def host(v, **kw):
        return gpu_ctx.tb_jacobian_batch_vars(m, *args, FRQ, ang, denliq=P["denliq"], denice=P["denice"], variables=v, **kw)
    htb, hvalid, hjac = host(variables)
    assert np.array_equal(htb, _np(tb), equal_nan=True) and np.array_equal(hvalid, _np(valid))
    assert sorted(hjac) == sorted(KEYS)
    for k in KEYS:
        assert np.array_equal(hjac[k], _np(jac[k]), equal_nan=True), k
    bare = host(variables, thickness=False)[2]
    assert "dtb_ddz" not in bare and all(np.array_equal(bare[k], hjac[k], equal_nan=True) for k in bare)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(MwrtError) as ei:
        host(JacVariables(0, 0, 5, 0))
    assert ei.value.code == -1
    assert torch.cuda.mem_get_info()[0] == free0
    host(variables)
    assert torch.cuda.mem_get_info()[0] == free0


def test_repeat_call_allocates_nothing(gpu_ctx):
    """After one warm-up call a variables call with the same shapes and the same buffers leaves the free device memory
    unchanged -- on the large-LDS launch as well (cloudy, 385 levels)."""
    m = sp.get_model("R24")
    ang = ANG[GOOD]
    for nlev in (180, 385):
        P = cloudy_profiles(nlev, 4, 61)
        arrs = {k: _dev(P[k]) for k in P}
        opts = dict(dtype=torch.float64, device="cuda")
        tb = torch.empty((4, len(ang), 3), **opts)
        jac = [torch.empty((4, len(ang), 3, nlev), **opts) for _ in range(4)]
        valid = torch.empty(4, dtype=torch.uint8, device="cuda")

        def call():
            gpu_ctx.tb_jacobian_batch_vars_device(
                m, 4, nlev, *(arrs[k].data_ptr() for k in ("z", "p", "t", "rh")), FRQ, ang, tb.data_ptr(), jac[0].data_ptr(),
                jac[1].data_ptr(), valid.data_ptr(), d_denliq=arrs["denliq"].data_ptr(), d_denice=arrs["denice"].data_ptr(),
                d_dtb_dliq=jac[2].data_ptr(), d_dtb_dice=jac[3].data_ptr(), variables=JacVariables(2, 1, 1, 0), stream=_cur())
            torch.cuda.synchronize()
        call()
        first = [j.clone() for j in jac]
        free0 = torch.cuda.mem_get_info()[0]
        call()
        assert torch.cuda.mem_get_info()[0] == free0, nlev
        assert all(torch.equal(a, b) for a, b in zip(first, jac))


def wrapper_errors():
    """jacobians_batch on three 40-level RTTOV-style profiles at two zenith angles with liquid, against end-to-end
    autograd in the wrapper's variables: the largest error per column kind, of the column's largest sum of absolute
    terms (from the chained reference)."""
    from mwr_fast_forward_operators_and_lbls_amd import pyrtlib_processing as pp, rttov_gb_wrapper as rw
    from test_kmatrix_variables_cpu import rttov_profiles
    profs = rttov_profiles((0.0, 70.8, 0.0), nlev=40)
    frqs = rw.HATPRO_FRQS[[0, 3, 6, 9, 13]]
    d = rw.jacobians_batch(profs, "R24", frqs, liquid=True)
    z, p, t, rh, elev = rw.to_lbl_inputs(profs)
    m = sp.get_model("R24")
    out = {"dtb_dt": 0.0, "dtb_dh": 0.0, "dtb_dliq": 0.0}
    for i, pr_ in enumerate(profs):
        den = pp.cloud_density_g_m3(pr_["liquid"][::-1], p[i], t[i])
        want = kv.end_to_end(m, z[i], p[i], t[i], rh[i], den, None, frqs, elev[i:i + 1], (2, 1, 1))
        K = cr.k_matrix_cloudy_rh(m, z[i], p[i], t[i], rh[i], den, None, frqs, elev[i:i + 1])
        _, scale = kv.chain(K, p[i], t[i], rh[i], den, None, (2, 1, 1))
        for got, key in zip(d, out):
            g = got[i][::-1].T[None]                          # [nlev top -> ground][nf] -> [1][nf][nlev ground -> top]
            out[key] = max(out[key], float(kv.scaled_row_errors(g, want[key], scale[key]).max()))
        assert np.abs(d[2][i]).max() > 1e3
    return out, profs, d


def test_wrapper_jacobians_batch_on_the_gpu(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd import rttov_gb_wrapper as rw
    err, profs, (d_t, d_q, d_l) = wrapper_errors()
    print(err)
    assert all(v <= TOL_K_ROW for v in err.values()), err
    assert d_t.shape == d_q.shape == d_l.shape == (3, 40, 5)
    for i in range(3):
        jac = rw.parse_jacobians(rw.format_jacobians(profs[i]["p"], d_t[i], d_q[i], d_l[i]), 40, 5)
        assert np.allclose(jac[:, :, 0], profs[i]["p"][:, None], atol=5e-5)
        for col, want in ((1, d_t[i]), (2, d_q[i]), (3, d_l[i])):
            assert np.allclose(jac[:, :, col], want, rtol=1e-10, atol=0)       # %18.10E: eleven significant digits
