"""The spectroscopic-parameter Jacobian on the device (include/mwrt.h mwrt_tb_param_jacobian_batch_device)
against its exact reference (tests/param_reference.py: torch autograd of the oracle's formulas with table entries as
leaves, on the CPU), column by column: every entry, no mask and no floor.

The bar is that of the K-matrix rows: 1e-8 of a column's largest |entry| over the profile's (elevation,
frequency) -- the same arithmetic, summed over the levels.  A parameter the model's modes do not read gives exactly 0.0."""
import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import _native, instrument, sensitivity, spectroscopy as sp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
prf = pytest.importorskip("param_reference")

from test_jacobian_device_edges import frequencies, k_matrix_device, profiles, tables  # noqa: E402
from test_tl_oracle import CASES, edge_profile  # noqa: E402

TOL_COL = 1e-8
ELEV = np.array([90.0, 30.0, 4.2, 179.0])


def _cur():
    return torch.cuda.current_stream().cuda_stream


def _dev(P):
    return [torch.tensor(np.ascontiguousarray(P[k]), dtype=torch.float64, device="cuda") for k in ("z", "p", "t", "rh")]


def ids_of(params):
    return [(_native.PARAM_FIELDS[name], line) for name, line in params]


def device_kb(ctx, m, P, frq, ang, params, want_tb=True):
    z, p, t, rh = _dev(P)
    nprof, nlev = z.shape
    opts = dict(dtype=torch.float64, device="cuda")
    tb = torch.full((nprof, len(ang), len(frq)), -7.0, **opts)
    kb = torch.full((nprof, len(ang), len(frq), len(params)), -7.0, **opts)
    valid = torch.full((nprof,), 9, dtype=torch.uint8, device="cuda")
    ctx.tb_param_jacobian_device(m, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang,
                                 ids_of(params), kb.data_ptr(), valid.data_ptr(), d_tb=tb.data_ptr() if want_tb else None,
                                 stream=_cur())
    torch.cuda.synchronize()
    return tb.cpu().numpy(), kb.cpu().numpy(), valid.cpu().numpy()


def unread(m, name):
    return (m.h2o_shift_mode == 0 and name in ("h2o_sh", "h2o_shs")) or \
           (m.o2_mix_mode == 0 and name in ("o2_g0", "o2_g1", "o2_dnu0", "o2_dnu1"))


def column_errors(m, P, frq, ang, params, kb, tb):
    """Per profile and column: max |got - want| / max |want| over (elevation, frequency); unread columns must be 0.0."""
    worst = {}
    for i in range(P["z"].shape[0]):
        tb_ref, kb_ref = prf.param_jacobian(m, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], frq, ang, params)
        assert np.abs(tb[i] - tb_ref).max() <= 1e-8, i
        for q, (name, line) in enumerate(params):
            got, want = kb[i, :, :, q], kb_ref[:, :, q]
            if unread(m, name):
                assert (got == 0.0).all() and (want == 0.0).all(), (i, name, line)
                continue
            scale = np.abs(want).max()
            err = np.abs(got - want).max() / scale if scale > 0 else (0.0 if (got == 0.0).all() else np.inf)
            worst[(name, line)] = max(worst.get((name, line), 0.0), err)
    return worst


def check(ctx, m, P, frq, ang, params, what):
    tb, kb, valid = device_kb(ctx, m, P, frq, ang, params)
    assert (valid == 1).all(), what
    worst = column_errors(m, P, frq, ang, params, kb, tb)
    top = max(worst.items(), key=lambda kv: kv[1])
    print(f"{what}: largest column error {top[1]:.2e} at {top[0]}")
    bad = {k: v for k, v in worst.items() if not v <= TOL_COL}
    assert not bad, (what, bad)
    return worst


def short_params(m, sd_line=None):
    """The scalars, every field at its first line, the speed-dependent line for the width and shift fields, three [*]."""
    out = [q for q in prf.test_params(m, sd_line) if q[1] == 0]
    if sd_line is not None:
        out += [(n, int(sd_line)) for n in ("h2o_w0", "h2o_x", "h2o_sh", "h2o_shs")]
    return out + [("h2o_w0", -1), ("o2_w300", -1), ("o2_y1", -1)]


# ---- 1. against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_field_first_last_sd_and_all_lines(gpu_ctx, case):
    """The four families and the fuzzed tables: the edge profile (a dry level, a dry block, a repeated level) and a second
    one with zero-thickness and 1e-6-km layers, eight frequencies, four elevations, every field at its first line, its
    last line, the speed-dependent line and [*]."""
    m, sd_frq = tables(case)
    sd_line = None
    if case.startswith("fuzz"):
        sd_line = int(np.argmin(np.abs(np.asarray(m.h2o["fl"]) + 0.3 - sd_frq)))
    frq = frequencies(8, sd_frq)
    z, p, t, rh = edge_profile()
    Q = profiles(30, 5)
    P = {k: np.stack([a, Q[k][0]]) for k, a in zip(("z", "p", "t", "rh"), (z, p, t, rh))}
    check(gpu_ctx, m, P, frq, ELEV, prf.test_params(m, sd_line), case)


@pytest.mark.parametrize("nlev,nf", [(2, 1), (64, 7), (65, 8), (180, 15)])
def test_level_and_frequency_seams(gpu_ctx, nlev, nf):
    """One layer; the 64-level wave / slab seam on both sides; the workload's 180 levels; the tangent kernel's frequency
    tails (nf 1, 7, 8, 15)."""
    m, sd_frq = tables("R20SD")
    sd_line = int(np.argmax(np.asarray(m.h2o["w2"]) > 0))
    Q = profiles(nlev, 11 + nlev)
    P = {k: v[:2] for k, v in Q.items()}
    check(gpu_ctx, m, P, frequencies(nf, sd_frq, rot=1), np.array([90.0, 4.2]), short_params(m, sd_line), f"nlev {nlev} nf {nf}")


def test_1024_levels(gpu_ctx):
    m, sd_frq = tables("fuzz2")
    Q = profiles(1024, 3)
    P = {k: v[:1] for k, v in Q.items()}
    check(gpu_ctx, m, P, np.array([22.235, 60.3061]), np.array([90.0, 4.2]), short_params(m), "1024 levels")


def test_64_angles(gpu_ctx):
    m, sd_frq = tables("R17")
    Q = profiles(30, 9)
    P = {k: v[:1] for k, v in Q.items()}
    ang = np.concatenate([np.linspace(4.2, 90.0, 40), np.linspace(91.0, 175.8, 24)])
    check(gpu_ctx, m, P, np.array([183.31]), ang, short_params(m), "64 angles")


# ---- 2. the TBs are the K-matrix entry's --------------------------------------------------------------------------------
def test_tb_equals_the_k_matrix_entrys(gpu_ctx):
    """Both kernels form the TB by the same statements from the same absorption arrays (k_absorb_tl's); the header promises
    1e-8 K.  Whether the bits agree too is printed, not asserted (it is the compiler's choice of contractions)."""
    m, sd_frq = tables("R20SD")
    P = profiles(180, 21, extreme=True)
    frq, ang = frequencies(14, sd_frq), np.array([90.0, 30.0, 4.2])
    tb, kb, valid = device_kb(gpu_ctx, m, P, frq, ang, short_params(m))
    tb_k, valid_k, _ = k_matrix_device(gpu_ctx, m, P, frq, ang)
    assert np.array_equal(valid, valid_k)
    good = valid == 1
    assert good.any() and np.abs(tb[good] - tb_k[good]).max() <= 1e-8
    print("TB bits equal:", np.array_equal(tb, tb_k, equal_nan=True))


# ---- 3. invariance ----------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_order_or_company(gpu_ctx):
    m, sd_frq = tables("R20SD")
    params = short_params(m, int(np.argmax(np.asarray(m.h2o["w2"]) > 0)))[::3] + [("o2_x", 0), ("h2o_s1", -1)]
    frq, ang = np.array([22.235, sd_frq, 60.3061]), np.array([90.0, 4.2])
    Q = profiles(65, 4)
    one = {k: v[:1] for k, v in Q.items()}
    tb1, kb1, _ = device_kb(gpu_ctx, m, one, frq, ang, params)
    for nprof in (5, 300):
        rep = {k: np.concatenate([np.repeat(v[1:2], nprof - 1, axis=0), v[:1]]) for k, v in Q.items()}
        tbn, kbn, _ = device_kb(gpu_ctx, m, rep, frq, ang, params)
        assert np.array_equal(kbn[-1], kb1[0]) and np.array_equal(tbn[-1], tb1[0]), nprof
        assert np.array_equal(kbn[0], kbn[nprof - 2])
    assert np.array_equal(device_kb(gpu_ctx, m, one, frq, ang, params)[1], kb1)                    # a repeat call
    assert np.array_equal(device_kb(gpu_ctx, m, one, frq, ang, params[::-1])[1][..., ::-1], kb1)   # the list reversed
    for q, par in enumerate(params):                                                                # each alone
        tba, kba, _ = device_kb(gpu_ctx, m, one, frq, ang, [par])
        assert np.array_equal(kba[..., 0], kb1[..., q]), par
        assert np.array_equal(tba, tb1)
    # without d_tb the columns are the same
    assert np.array_equal(device_kb(gpu_ctx, m, one, frq, ang, params, want_tb=False)[1], kb1)


def test_host_entry_returns_the_device_entrys_bits(gpu_ctx):
    m, sd_frq = tables("R98")
    params = short_params(m)
    P = profiles(30, 8)
    P["t"][1, 4] = np.nan
    frq, ang = np.array([22.235, 118.7503]), np.array([90.0, np.nan, 4.2])
    tb, kb, valid = device_kb(gpu_ctx, m, P, frq, ang, params)
    tb_h, kb_h, valid_h = gpu_ctx.tb_param_jacobian(m, P["z"], P["p"], P["t"], P["rh"], frq, ang, ids_of(params))
    assert np.array_equal(valid, valid_h) and list(valid) == [1, 0, 1]
    assert np.array_equal(tb, tb_h, equal_nan=True) and np.array_equal(kb, kb_h, equal_nan=True)
    assert np.isnan(kb[1]).all() and np.isnan(tb[1]).all()
    assert np.isnan(kb[0, 1]).all() and np.isnan(tb[0, 1]).all() and np.isfinite(kb[0, [0, 2]]).all() and np.isfinite(tb[0, [0, 2]]).all()


# ---- 4. NaN, valid, refusals, capture -----------------------------------------------------------------------------------
def test_nan_and_valid_rules(gpu_ctx):
    m, _ = tables("R20")
    params = short_params(m)
    P = profiles(65, 6)
    Pn = {k: np.concatenate([v, v[:2]]) for k, v in P.items()}            # five profiles
    Pn["rh"][1, 64] = np.nan
    Pn["z"][3, 0] = np.nan
    frq, ang = np.array([60.3061, 183.31]), np.array([np.nan, 30.0])
    tb, kb, valid = device_kb(gpu_ctx, m, Pn, frq, ang, params)
    assert list(valid) == [1, 0, 1, 0, 1]
    for i in (1, 3):
        assert np.isnan(kb[i]).all() and np.isnan(tb[i]).all()
    for i in (0, 2, 4):
        assert np.isnan(kb[i, 0]).all() and np.isnan(tb[i, 0]).all()
        assert np.isfinite(kb[i, 1]).all() and np.isfinite(tb[i, 1]).all()
    tb0, kb0, _ = device_kb(gpu_ctx, m, {k: v[:1] for k, v in P.items()}, frq, np.array([30.0]), params)
    assert np.array_equal(kb[0, 1], kb0[0, 0])
    # a negative absorption coefficient (negative H2O line strengths): valid 2, rows NaN, as the K-matrix entry
    import dataclasses
    h2o = {k: np.array(v, dtype=float) for k, v in m.h2o.items()}
    h2o["s1"] *= -1.0
    neg = dataclasses.replace(m, name="neg", h2o=h2o)
    one = {k: v[:1] for k, v in P.items()}
    tb2, kb2, valid2 = device_kb(gpu_ctx, neg, one, np.array([22.235]), np.array([90.0]), [("h2o_cf", 0), ("o2_y0", 2)])
    tbk, validk, _ = k_matrix_device(gpu_ctx, neg, one, np.array([22.235]), np.array([90.0]))
    assert list(valid2) == list(validk) == [2]
    assert np.isnan(kb2).all() and np.isnan(tb2).all()


def test_refusals_write_nothing(gpu_ctx):
    m, _ = tables("R20")
    P = {k: v[:1] for k, v in profiles(30, 2).items()}
    z, p, t, rh = _dev(P)
    kb = torch.full((1, 1, 1, 300), -7.0, dtype=torch.float64, device="cuda")
    valid = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    n_h2o, n_o2 = len(m.h2o["fl"]), len(m.o2["f"])
    F = _native.PARAM_FIELDS

    def call(params, frq=(22.235,), ang=(90.0,), nprof=1):
        gpu_ctx.tb_param_jacobian_device(m, nprof, 30, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), np.array(frq),
                                         np.array(ang), params, kb.data_ptr(), valid.data_ptr(), stream=_cur())
    for bad in ([(24, 0)], [(-1, 0)], [(F["h2o_cf"], 1)], [(F["o2_x"], -1)], [(F["h2o_w0"], n_h2o)], [(F["h2o_w0"], -2)],
                [(F["o2_y0"], n_o2)], [(F["h2o_cf"], 0)] * 257, []):
        with pytest.raises(_native.MwrtError) as ei:
            call(bad)
        assert ei.value.code == -1, bad
    with pytest.raises(_native.MwrtError) as ei:
        call([(F["h2o_cf"], 0)], frq=(np.nan,))
    assert ei.value.code == -1
    call([(F["h2o_cf"], 0)], nprof=0)                                      # MWRT_OK, nothing to do
    call([(F["h2o_cf"], 0)] * 256, nprof=0)
    torch.cuda.synchronize()
    assert (kb.cpu().numpy() == -7.0).all() and valid.item() == 9


def test_capture_and_replay(gpu_ctx):
    m, sd_frq = tables("R20SD")
    params = ids_of(short_params(m))
    P = profiles(65, 12)
    z, p, t, rh = _dev(P)
    frq, ang = np.array([22.235, sd_frq]), np.array([90.0, 4.2])
    opts = dict(dtype=torch.float64, device="cuda")
    tb = torch.zeros((3, 2, 2), **opts)
    kb = torch.zeros((3, 2, 2, len(params)), **opts)
    valid = torch.zeros((3,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        def run():
            gpu_ctx.tb_param_jacobian_device(m, 3, 65, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, params,
                                             kb.data_ptr(), valid.data_ptr(), d_tb=tb.data_ptr(),
                                             stream=torch.cuda.current_stream().cuda_stream)
        run()                                                              # the warm-up: workspace and device copies
        s.synchronize()
        want_kb, want_tb = kb.clone(), tb.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            run()
        kb.zero_(); tb.zero_(); valid.zero_()
        g.replay()
        s.synchronize()
    assert torch.equal(kb, want_kb) and torch.equal(tb, want_tb) and valid.tolist() == [1, 1, 1]


# ---- 5. consistency with the product's own forward ------------------------------------------------------------------------
def test_columns_equal_central_differences_of_the_forward_entry(gpu_ctx):
    """4 profiles x 180 levels x 14 channels x 7 elevations, about 30 parameters: mwrt_tb_batch_device on models registered
    with one entry perturbed (relative step 1e-4) against the K_b column, 1e-5 of the column's scale (the step error of the
    quotient, as in tests/test_param_reference.py)."""
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr
    m = sp.get_model("R24")
    frq = np.array([22.24, 23.04, 23.84, 25.44, 26.24, 27.84, 31.4, 51.26, 52.28, 53.86, 54.94, 56.66, 57.3, 58.0])
    ang = np.array([90.0, 42.0, 30.0, 19.2, 10.2, 5.4, 4.2])
    S = pr.synthetic_profiles(4, 17, nlev=180)
    P = {k: np.ascontiguousarray(S[k]) for k in ("z", "p", "t", "rh")}
    names = ["h2o_cf", "h2o_cs", "h2o_xcf", "h2o_xcs", "o2_x", "o2_wb300", "n2_l"]
    params = [(n, 0) for n in names] + [(n, 0) for n in ("h2o_s1", "h2o_b2", "h2o_w0", "h2o_x", "h2o_w0s", "h2o_xs")] + \
             [(n, k) for n in ("o2_s300", "o2_be", "o2_w300", "o2_y0", "o2_y1") for k in (1, 5, 9)] + \
             [("h2o_w0", -1), ("o2_w300", -1), ("o2_y0", -1), ("o2_s300", -1)]
    tb, kb, valid = device_kb(gpu_ctx, m, P, frq, ang, params)
    assert (valid == 1).all()
    z, p, t, rh = _dev(P)
    out = torch.empty((4, 7, 14), dtype=torch.float64, device="cuda")
    vd = torch.empty((4,), dtype=torch.uint8, device="cuda")

    def forward(tab):
        gpu_ctx.tb_batch_device(tab, 4, 180, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, ang, out.data_ptr(),
                                vd.data_ptr(), stream=_cur())
        torch.cuda.synchronize()
        return out.cpu().numpy()
    h = 1e-4
    worst = 0.0
    for q, (name, line) in enumerate(params):
        b = prf.table_value(m, name, line)
        fd = (forward(prf.perturbed_tables(m, name, line, 1.0 + h)) - forward(prf.perturbed_tables(m, name, line, 1.0 - h))) / (2 * h * b)
        col = kb[..., q]
        err = np.abs(col - fd).max() / np.abs(col).max()
        worst = max(worst, err)
        print(f"{name}[{line}]: {err:.2e}")
        assert err <= 1e-5, (name, line, err)
    print("worst", worst)


# ---- 6. the instrument operator and the covariance -------------------------------------------------------------------
def test_instrument_param_jacobian_and_model_error_covariance(gpu_ctx, monkeypatch):
    monkeypatch.setattr(_native, "default_context", lambda device_id=0: gpu_ctx)
    m = sp.get_model("R20")
    inst = instrument.Instrument([22.24, 31.4, 51.26, 58.0], [90.0, 10.2], beam=3.0, band=0.2, n_beam=3, n_band=3)
    P = profiles(65, 14)
    z, p, t, rh = _dev(P)
    specs = ["h2o_cf", "h2o_w0[0]", "o2_w300[*]", "o2_y0[3]", "o2_x", "n2_l"]
    recs = sensitivity.parse_params(m, specs)
    tb_q, kb_q, valid = sensitivity.param_jacobian(m, z, p, t, rh, inst.frq_q, inst.elev_q, recs)
    tb_ch, kb_ch, valid_ch = inst.param_jacobian(m, z, p, t, rh, specs)
    D = inst.dense()
    want = np.einsum("oi,pik->pok", D, kb_q.cpu().numpy().reshape(3, inst.m_in, len(recs)))
    got = kb_ch.cpu().numpy().reshape(3, inst.m_out, len(recs))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(tb_ch.cpu().numpy().reshape(3, -1) - tb_q.cpu().numpy().reshape(3, -1) @ D.T).max() <= 1e-12 * 300
    # relative scaling, then K_b S_b K_b^T
    kb_rel = sensitivity.scale_relative(kb_ch, recs)
    vals = np.array([q.value for q in recs])
    assert np.array_equal(kb_rel.cpu().numpy(), kb_ch.cpu().numpy() * vals)
    rng = np.random.default_rng(3)
    A = rng.normal(size=(len(recs), len(recs))) * 0.02
    sb_full, sb_var = A @ A.T, rng.uniform(1e-4, 4e-4, len(recs))
    k = kb_rel.cpu().numpy().reshape(3, inst.m_out, len(recs))
    for sb, ref in ((sb_var, np.einsum("pik,k,pjk->pij", k, sb_var, k)), (sb_full, np.einsum("pik,kl,pjl->pij", k, sb_full, k))):
        cov = sensitivity.model_error_covariance(kb_rel, sb).cpu().numpy()
        assert cov.shape == (3, inst.m_out, inst.m_out)
        assert np.abs(cov - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(cov, cov.transpose(0, 2, 1))
        for c in cov:
            assert np.linalg.eigvalsh(c).min() >= -1e-12 * np.abs(c).max()
        mean = sensitivity.model_error_covariance(kb_rel, sb, reduce="mean").cpu().numpy()
        assert np.abs(mean - ref.mean(axis=0)).max() <= 1e-12 * np.abs(ref).max()
    inst.close()
