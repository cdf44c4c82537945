"""mwrt_oe_step_device (include/mwrt.h) on the GPU against tests/oe_reference.py, every output of every case.

Tolerance (derived, not measured): Cholesky + solves are backward stable, error <~ c m eps cond(G); with c = 64, m <= 140
and cond_2(G) <= 1e4 (asserted on the reference's G for every case) that is ~1e-8.  x_new is held to 1e-8 of max |x_ref - xa|
per block, post_var to 1e-8 of max diag Sa per block, chi2 and dfs to 1e-8 max(1, |ref|).  No mask, no floor.

Shapes (nlev, nblk, m) are oe_reference.SHAPES.  What they reach is asserted by
test_oe_shape_coverage.py::test_the_shapes_reach_what_they_are_for against the code's own LDS plan and dispatch rule, and
that test is the authority: k_oe_step<1 .. 5> with m = 32 k and 32 k + 1 on both sides of every tile edge, m = 1 and the
m limit 140, one to four K blocks, both sides of the seams of wave 0's solve registers (m = 64 | 65, 128 | 129), both
sides of the first raise of the kernel's LDS limit (m = 69 | 70 at n = 130), the two shapes whose x - xa outgrows the panel
buffers it aliases (n = 2100 at one tile, 3636 at two), the wave seams of the level axis (63 / 64 / 65) and a panel
remainder.  Rows are dropped at m = 98 and, on the tile and register seams, at m = 65 (oe_reference.SEAM_DROPS)."""
import ctypes

import numpy as np
import pytest

import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OUT_KEYS = ("x_new", "status", "chi2", "dfs", "post_var", "nobs")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


def run_device(ctx, case, want=OUT_KEYS, stream=None, sync=True, **kw):
    """One mwrt_oe_step_device call on a case of oe_reference.make_case -> dict of NumPy outputs (None where not asked
    for); outputs are pre-filled with a sentinel so an entry the kernel leaves unwritten shows."""
    k = [_dev(b) for b in case["k"]]
    nprof, m, nlev = k[0].shape
    nblk = len(k)
    x, xa, sa, se, y, fx = (_dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(x_new=torch.full((nprof, nblk, nlev), -7.0, **f64), status=torch.full((nprof,), 9, dtype=torch.uint8, device="cuda"),
               chi2=torch.full((nprof,), -7.0, **f64), dfs=torch.full((nprof,), -7.0, **f64),
               post_var=torch.full((nprof, nblk, nlev), -7.0, **f64),
               nobs=torch.full((nprof,), -7, dtype=torch.int32, device="cuda"))
    ptr = lambda key: out[key].data_ptr() if key in want else None   # noqa: E731
    ctx.oe_step_device(nprof, nlev, m, [b.data_ptr() for b in k], x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(),
                       y.data_ptr(), fx.data_ptr(), ptr("x_new"), ptr("status"), d_chi2=ptr("chi2"), d_dfs=ptr("dfs"),
                       d_post_var=ptr("post_var"), d_nobs=ptr("nobs"), xa_per_profile=case["xa"].ndim == 3,
                       se_full=case["se"].ndim == 2, stream=_cur() if stream is None else stream, **kw)
    if sync:
        torch.cuda.synchronize()
    return {key: (out[key].cpu().numpy() if key in want else None) for key in OUT_KEYS}


def check_against_reference(got, ref, case, label):
    assert got["status"].tolist() == ref["status"].tolist(), label
    assert got["nobs"].tolist() == ref["nobs"].tolist(), label
    ok = ref["status"] == 1
    assert ok.any() and np.nanmax(ref["cond"]) <= oer.COND_MAX, (label, ref["cond"])
    err = oer.block_errors(got, ref, case)
    print(label, err)
    assert all(np.isfinite(got[k][ok]).all() for k in ("x_new", "chi2", "dfs", "post_var")), label
    assert all(v <= oer.TOL for v in err.values()), (label, err)
    return err


_refs = {}


def case_and_reference(nlev, nblk, m, se_full, xa_pp, nprof):
    key = (nlev, nblk, m, se_full, xa_pp, nprof)
    if key not in _refs:
        case = oer.make_case(nlev, nblk, m, nprof=nprof, se_full=se_full, xa_per_profile=xa_pp)
        _refs[key] = (case, oer.oe_step_reference(**case))
    return _refs[key]


@pytest.mark.parametrize("nlev,nblk,m", oer.SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in oer.SHAPES])
@pytest.mark.parametrize("se_full,xa_pp", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["diag-shared", "full-shared", "diag-perprofile", "full-perprofile"])
def test_every_output_against_the_reference(gpu_ctx, nlev, nblk, m, se_full, xa_pp):
    nprof = 3 if nlev >= 180 else 4
    case, ref = case_and_reference(nlev, nblk, m, se_full, xa_pp, nprof)
    got = run_device(gpu_ctx, case)
    check_against_reference(got, ref, case, (nlev, nblk, m, se_full, xa_pp))


def _copy(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else [b.copy() for b in v]) for k, v in case.items()}


@pytest.mark.parametrize("what", ["y", "fx", "k", "se-diag", "se-full"])
def test_dropped_rows_equal_rows_deleted(gpu_ctx, what):
    nlev, nblk, m, nprof = 65, 2, 98, 4
    base, _ = case_and_reference(nlev, nblk, m, what == "se-full", False, nprof)
    clean = run_device(gpu_ctx, base)
    for row in (0, m - 1, 41):
        case = _copy(base)
        if what == "k":
            case["k"][1][1, row, 64] = np.nan                  # one element of one block, profile 1
        elif what == "se-diag":
            case["se"][row] = np.inf                           # shared: every profile drops the row
        elif what == "se-full":
            case["se"][row, (row + 5) % m] = np.nan            # one element of row `row` of the full matrix
        else:
            case[what][1, row] = np.nan
        ref = oer.oe_step_reference(**case)
        shared = what.startswith("se")
        assert ref["nobs"].tolist() == ([m - 1] * nprof if shared else [m, m - 1, m, m])
        got = run_device(gpu_ctx, case)
        check_against_reference(got, ref, case, (what, row))
        if not shared:                                         # the neighbours never see it: bit for bit
            for i in (0, 2, 3):
                for key in OUT_KEYS:
                    assert np.array_equal(got[key][i], clean[key][i]), (what, row, i, key)


@pytest.mark.parametrize("pattern", list(oer.SEAM_DROPS))
@pytest.mark.parametrize("what", ["y", "k"])
def test_dropped_rows_at_the_seams_equal_rows_deleted(gpu_ctx, what, pattern):
    """m = 65: row 64 is the only row of the third tile and the only entry of wave 0's second register.  Profile 1 loses
    the last row of a tile, the first of the next, a whole tile (32 rows of the identity in G), or every row but 64."""
    (nlev, nblk, m), nprof = oer.SEAM_SHAPE, 4
    dropped = oer.SEAM_DROPS[pattern]
    base, _ = case_and_reference(nlev, nblk, m, False, False, nprof)
    clean = run_device(gpu_ctx, base)
    case = oer.drop_rows(base, what, dropped, 1)
    ref = oer.oe_step_reference(**case)
    assert ref["nobs"].tolist() == [m, m - len(dropped), m, m]
    got = run_device(gpu_ctx, case)
    check_against_reference(got, ref, case, (what, pattern))
    print((what, pattern), "profile 1 alone", oer.block_errors(oer.one_profile(got, 1), oer.one_profile(ref, 1), case))
    for i in (0, 2, 3):                                       # the neighbours never see it: bit for bit
        for key in OUT_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (what, pattern, i, key)


def test_status_values_and_untouched_neighbours(gpu_ctx):
    nlev, nblk, m, nprof = 65, 2, 98, 5
    base, _ = case_and_reference(nlev, nblk, m, False, True, nprof)
    clean = run_device(gpu_ctx, base)
    case = _copy(base)
    for b in case["k"]:
        b[1] = np.nan                                          # what an invalid profile of the Jacobian call looks like
    case["fx"][1] = np.nan
    case["x"][3, 1, 17] = np.nan
    got = run_device(gpu_ctx, case)
    ref = oer.oe_step_reference(**case)
    assert got["status"].tolist() == ref["status"].tolist() == [1, 3, 1, 0, 1]
    assert got["nobs"].tolist() == [m, 0, m, 0, m]
    assert np.array_equal(got["x_new"][1], case["xa"][1])      # the prior, bit for bit
    assert got["chi2"][1] == 0.0 and got["dfs"][1] == 0.0
    assert np.array_equal(got["post_var"][1].ravel(), np.diag(case["sa"]))
    assert np.isnan(got["x_new"][3]).all() and np.isnan(got["post_var"][3]).all()
    assert np.isnan(got["chi2"][3]) and np.isnan(got["dfs"][3])
    for i in (0, 2, 4):
        for key in OUT_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (i, key)
    # NaN in xa alone is status 0 as well
    case = _copy(base)
    case["xa"][2, 0, 64] = np.inf
    got = run_device(gpu_ctx, case)
    assert got["status"].tolist() == [1, 1, 0, 1, 1] and np.isnan(got["x_new"][2]).all()
    # an indefinite G: a negative variance larger than K Sa K^T's diagonal
    case = _copy(base)
    case["se"][40] = -1e9
    got = run_device(gpu_ctx, case)
    assert got["status"].tolist() == [2] * nprof and got["nobs"].tolist() == [m] * nprof
    assert np.isnan(got["x_new"]).all() and np.isnan(got["chi2"]).all() and np.isnan(got["dfs"]).all()
    assert np.isnan(got["post_var"]).all()


def test_outputs_do_not_depend_on_the_batch(gpu_ctx):
    nlev, nblk, m = 65, 2, 98
    big = oer.make_case(nlev, nblk, m, nprof=300)
    got300 = run_device(gpu_ctx, big)
    again = run_device(gpu_ctx, big)
    for key in OUT_KEYS:
        assert np.array_equal(got300[key], again[key], equal_nan=True), key
    assert (got300["status"] == 1).all()
    for nprof in (1, 5):
        sub = dict(big, k=[b[:nprof] for b in big["k"]], x=big["x"][:nprof], y=big["y"][:nprof], fx=big["fx"][:nprof])
        got = run_device(gpu_ctx, sub)
        for key in OUT_KEYS:
            assert np.array_equal(got[key], got300[key][:nprof]), (nprof, key)
    # the last profile of the large batch as a batch of one
    j = 299
    one = dict(big, k=[b[j:j + 1] for b in big["k"]], x=big["x"][j:j + 1], y=big["y"][j:j + 1], fx=big["fx"][j:j + 1])
    got = run_device(gpu_ctx, one)
    for key in OUT_KEYS:
        assert np.array_equal(got[key][0], got300[key][j]), key


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_optional_outputs_leave_x_new_unchanged(gpu_ctx, se_full):
    case, _ = case_and_reference(65, 2, 98, se_full, False, 4)
    full = run_device(gpu_ctx, case)
    for want in (("x_new", "status"), ("x_new", "status", "chi2"), ("x_new", "status", "dfs", "nobs"),
                 ("x_new", "status", "post_var")):
        got = run_device(gpu_ctx, case, want=want)
        assert np.array_equal(got["x_new"], full["x_new"]) and np.array_equal(got["status"], full["status"]), want
        for key in want:
            assert np.array_equal(got[key], full[key]), (want, key)
    # a record that ends after d_status: the optional fields are absent (the next test fills them with wild values)
    got = run_device(gpu_ctx, case, want=("x_new", "status"), struct_size=_native.MwrtOeStep.d_chi2.offset)
    assert np.array_equal(got["x_new"], full["x_new"]) and got["status"].tolist() == [1] * 4


def test_short_record_ignores_the_fields_beyond_it(gpu_ctx):
    case, _ = case_and_reference(33, 1, 17, False, False, 4)
    full = run_device(gpu_ctx, case)
    k = [_dev(b) for b in case["k"]]
    x, xa, sa, se, y, fx = (_dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
    x_new = torch.empty_like(x)
    status = torch.zeros(4, dtype=torch.uint8, device="cuda")
    rec = _native.MwrtOeStep()
    rec.struct_size = _native.MwrtOeStep.d_chi2.offset
    rec.nblk = 1
    rec.d_k[0] = k[0].data_ptr()
    rec.d_x, rec.d_xa, rec.d_sa, rec.d_se, rec.d_y, rec.d_fx = (t.data_ptr() for t in (x, xa, sa, se, y, fx))
    rec.d_x_new, rec.d_status = x_new.data_ptr(), status.data_ptr()
    rec.d_chi2 = rec.d_dfs = rec.d_post_var = rec.d_nobs = 8         # not addresses: reading them as such would fault
    # ... whether the record ends at a field boundary or inside d_chi2 (a half-copied pointer would be written through)
    for size in (_native.MwrtOeStep.d_chi2.offset, _native.MwrtOeStep.d_chi2.offset + 4):
        rec.struct_size = size
        x_new.fill_(-7.0)
        status.zero_()
        rc = gpu_ctx._lib.mwrt_oe_step_device(gpu_ctx._handle, 4, 33, 17, ctypes.byref(rec), _native._stream(_cur()))
        assert rc == 0, gpu_ctx._lib.mwrt_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(x_new.cpu().numpy(), full["x_new"]) and status.cpu().tolist() == [1] * 4, size


def test_argument_refusals(gpu_ctx):
    case = oer.make_case(3, 3, 14, nprof=2)
    k = [_dev(b) for b in case["k"]]
    x, xa, sa, se, y, fx = (_dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
    x_new, status = torch.empty_like(x), torch.zeros(2, dtype=torch.uint8, device="cuda")
    base = dict(nprof=2, nlev=3, m=14, d_k=[b.data_ptr() for b in k], d_x=x.data_ptr(), d_xa=xa.data_ptr(),
                d_sa=sa.data_ptr(), d_se=se.data_ptr(), d_y=y.data_ptr(), d_fx=fx.data_ptr(), d_x_new=x_new.data_ptr(),
                d_status=status.data_ptr(), stream=_cur())

    def code(**change):
        with pytest.raises(MwrtError) as ei:
            gpu_ctx.oe_step_device(**dict(base, **change))
        return ei.value.code, str(ei.value)

    gpu_ctx.oe_step_device(**base)                                   # the unchanged call is accepted
    for name in ("d_x", "d_xa", "d_sa", "d_se", "d_y", "d_fx", "d_x_new", "d_status"):
        assert code(**{name: None})[0] == -1, name
    assert code(d_k=[k[0].data_ptr(), None, k[2].data_ptr()])[0] == -1
    assert code(d_k=[])[0] == -1 and code(d_k=[k[0].data_ptr()] * 5)[0] == -1        # nblk 0 and 5
    assert code(reserved=1)[0] == -1
    assert code(nlev=0)[0] == -1 and code(m=0)[0] == -1 and code(nprof=-1)[0] == -1
    assert code(struct_size=_native.MwrtOeStep.d_status.offset)[0] == -1             # ends before d_status
    assert code(struct_size=0)[0] == -1
    c, text = code(m=_native.OE_MAX_M + 1)
    assert c == -5 and str(_native.OE_MAX_M) in text
    c, text = code(nlev=1025)
    assert c == -5 and "1024" in text
    gpu_ctx.oe_step_device(**dict(base, nprof=0))                    # nothing to do is not an error
    torch.cuda.synchronize()


def test_repeat_call_allocates_nothing_and_orders_on_the_callers_stream(gpu_ctx):
    case, ref = case_and_reference(180, 2, 98, False, False, 3)
    first = run_device(gpu_ctx, case)
    k = [_dev(b) for b in case["k"]]
    x, xa, sa, se, y, fx = (_dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
    x_new, doubled = torch.empty_like(x), torch.empty_like(x)
    status = torch.zeros(3, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()

    def call(stream):
        gpu_ctx.oe_step_device(3, 180, 98, [b.data_ptr() for b in k], x.data_ptr(), xa.data_ptr(), sa.data_ptr(),
                               se.data_ptr(), y.data_ptr(), fx.data_ptr(), x_new.data_ptr(), status.data_ptr(), stream=stream)

    with torch.cuda.stream(side):                                    # warm-up of everything this test launches on `side`
        call(side.cuda_stream)
        torch.mul(x_new, 2.0, out=doubled)
        x_new.fill_(-7.0)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    call(side.cuda_stream)
    side.synchronize()
    assert torch.cuda.mem_get_info()[0] == before                    # hipMemGetInfo: the call took and freed nothing
    with torch.cuda.stream(side):
        x_new.fill_(-7.0)
        call(side.cuda_stream)
        torch.mul(x_new, 2.0, out=doubled)                           # consumed on the same stream: ordered behind the kernel
    side.synchronize()                                               # that stream alone, no device-wide wait
    assert np.array_equal(doubled.cpu().numpy(), 2.0 * first["x_new"])
    assert status.cpu().tolist() == [1] * 3


# ---- end to end: OneDVar on the real operator ----
def _retrieval_setup():
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    from mwr_fast_forward_operators_and_lbls_amd.autodiff import goff_gratch_es
    nprof, nlev = 4, 12
    P = pr.synthetic_profiles(nprof, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, nlev)).astype(int)           # 12 of the 180 levels, ground to ~12 km
    P = {k: np.ascontiguousarray(v[:, pick]) for k, v in P.items()}
    frq, elev = np.array([22.24, 31.4, 53.86]), np.array([90.0, 19.2])
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    lev = np.arange(nlev)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 3.0)
    sa = np.zeros((2 * nlev, 2 * nlev))
    sa[:nlev, :nlev] = 2.0 ** 2 * corr
    sa[nlev:, nlev:] = 0.1 ** 2 * corr
    se = np.full(6, 0.25)
    truth = torch.stack([t, rh], dim=1).contiguous()
    ov = retrieval.OneDVar("R24", frq, elev, _dev(sa), _dev(se), variables=JacVariables.of(humidity="rh"),
                           blocks=("t", "h"), xa=truth.clone())
    return ov, z, p, truth, sa, se, goff_gratch_es


def test_one_d_var_step_equals_the_step_assembled_on_the_host(gpu_ctx):
    ov, z, p, truth, sa, se, _ = _retrieval_setup()
    rng = np.random.default_rng(5)
    x = truth + _dev(rng.standard_normal(tuple(truth.shape)) * np.array([0.5, 0.02])[None, :, None])
    y = _dev(250.0 + rng.standard_normal((4, 2, 3)))
    y[2, 1, 0] = float("nan")                                        # one observation missing
    x_new, d = ov.step(z, p, x, y)
    torch.cuda.synchronize()
    # the same step from the K-matrix call's outputs on the host (the module's one route to that call, as step takes it)
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    zz, t, rh, _, _ = ov.physical(z, p, x)
    tb, valid, rows = retrieval._native_k_matrix("R24", zz, p, t, rh, None, None, ov.frq, ov.elev, ov.variables, ("t", "h"), _cur())
    torch.cuda.synchronize()
    assert valid.cpu().tolist() == [1] * 4
    case = dict(k=[rows[b].cpu().numpy().reshape(4, 6, 12) for b in ("t", "h")], x=x.cpu().numpy(),
                xa=truth.cpu().numpy(), sa=sa, se=se, y=y.cpu().numpy().reshape(4, 6), fx=tb.cpu().numpy().reshape(4, 6))
    ref = oer.oe_step_reference(**case)
    got = dict(x_new=x_new.cpu().numpy(), status=d["status"].cpu().numpy(), chi2=d["chi2"].cpu().numpy(),
               dfs=d["dfs"].cpu().numpy(), post_var=d["post_var"].cpu().numpy(), nobs=d["nobs"].cpu().numpy())
    assert got["nobs"].tolist() == [6, 6, 5, 6]
    check_against_reference(got, ref, case, "OneDVar.step")


def test_one_d_var_retrieve_closes_on_noise_free_observations(gpu_ctx):
    ov, z, p, truth, sa, se, _ = _retrieval_setup()
    rng = np.random.default_rng(6)
    lev = np.arange(12)
    bump = np.exp(-((lev - 3.0) / 4.0) ** 2)                        # a smooth departure from the prior
    x_true = truth + _dev(np.stack([3.0 * bump, 0.12 * bump])[None] * rng.uniform(0.5, 1.0, (4, 1, 1)))
    y, valid = ov.forward(z, p, x_true)
    assert valid.cpu().tolist() == [1] * 4
    sa_inv, xa = np.linalg.inv(sa), truth.cpu().numpy().reshape(4, -1)

    def residual_rms_and_cost(x):
        """RMS of F(x) - y over the batch, and per profile the cost Gauss-Newton descends:
        J = (y - F)^T Se^-1 (y - F) + (x - xa)^T Sa^-1 (x - xa)."""
        r = (ov.forward(z, p, x)[0] - y).cpu().numpy().reshape(4, -1)
        dx = x.cpu().numpy().reshape(4, -1) - xa
        return float(np.sqrt((r ** 2).mean())), (r ** 2 / se).sum(axis=1) + np.einsum("ij,jk,ik->i", dx, sa_inv, dx)

    tol = 0.05
    full = ov.retrieve(z, p, y, max_iter=10, tol=tol)
    n_it = int(full.iterations.max())
    assert full.converged.all() and 2 <= n_it < 10
    rms, cost = (list(v) for v in zip(residual_rms_and_cost(truth)))
    for it in range(1, n_it + 1):
        res = ov.retrieve(z, p, y, max_iter=it, tol=tol)
        r, j = residual_rms_and_cost(res.x)
        rms.append(r)
        cost.append(j)
    print("TB residual RMS per iteration:", rms)
    print("cost J per iteration and profile:", [c.tolist() for c in cost])
    assert torch.equal(res.x, full.x)
    assert rms[0] > np.sqrt(se[0])                                   # the prior does not already fit
    # Monotone in what the iteration descends: the cost J of every profile falls (or stays) at every step, the confirming
    # last one included.  The residual alone is not that quantity -- at the fixed point the prior term trades against it,
    # so it is stationary only to first order there -- but it must fall at every step that still moves the
    # state by tol sqrt(Sa_ii) or more, i.e. at all but the last, and the run must end below sqrt(Se).
    assert all((b <= a).all() for a, b in zip(cost, cost[1:])), cost
    assert all(b < a for a, b in zip(rms[:-1], rms[1:-1])), rms
    assert rms[-1] < np.sqrt(se[0]), rms
    assert (res.status == 1).all() and (res.x[:, 1] >= 0).all()
    assert (res.dfs > 0).all() and (res.dfs < 6).all() and (res.post_var <= _dev(np.diag(sa)).reshape(2, 12)).all()
