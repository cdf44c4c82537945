"""mwrt_oe_gain_device and mwrt_oe_product_device (include/mwrt.h) on the GPU against
tests/oe_char_reference.py, every output of every case.

Tolerance (derived, not measured; the argument of test_oe_step.py): Cholesky, inverse and solves are backward stable, error
<~ c m eps cond(G); with c = 64, m <= 140 and cond_2(G) <= 1e4 (asserted on the reference's G for every case) that is
~1e-8 = oe_reference.TOL.  Each output is compared in units of its own scale (oe_char_reference.char_errors), no mask, no
floor.  The product entry alone, on exact inputs, is held element by element to the forward bound of a length-m sum:
2 m eps (|gain|^T |K|)_jk, resp. 2 m eps (|Sa_jk| + (|gain|^T |W|)_jk).

Shapes (nlev, nblk, m) are oe_reference.SHAPES.  What they reach in the gain kernel is asserted by
test_oe_shape_coverage.py::test_the_shapes_reach_what_they_are_for against the code's own LDS plan and dispatch rule, and
that test is the authority: k_char_gain<1 .. 5> with both sides of every tile edge, m = 1 and the m limit, one to four K
blocks, and both sides of the first raise of the kernel's LDS limit (m = 64 | 65).  For the product kernel the list holds
n = 128 (its exact tile) and 130 (tile + 2), the panel remainders and a block seam inside a tile.  At n = 2048 the products
are taken through two row windows instead of one 134-MB result per call, beyond it through three windows of 64 rows
(_windows).  Rows are dropped at m = 98 and, on the tile seams, at m = 65 (oe_reference.SEAM_DROPS)."""
import ctypes

import numpy as np
import pytest

import oe_char_reference as ocr
import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError
from test_oe_step import run_device as run_step

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GAIN_KEYS = ("gain", "ksa", "keep", "avk_diag", "dfs_block", "noise_var", "smooth_var", "status", "nobs")
FLOAT_KEYS = ("gain", "ksa", "avk_diag", "dfs_block", "noise_var", "smooth_var")
COMBOS = [(False, False), (True, False), (False, True), (True, True)]
COMBO_IDS = ["diag-shared", "full-shared", "diag-perprofile", "full-perprofile"]
SHAPE_IDS = [f"{a}-{b}-{c}" for a, b, c in oer.SHAPES]
SENTINEL = -7.0


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


def upload(case):
    d = {key: _dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx")}
    d["k"] = [_dev(b) for b in case["k"]]
    return d


def gain_buffers(nprof, nblk, nlev, m):
    n = nblk * nlev
    f64, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.uint8, device="cuda")
    return dict(gain=torch.full((nprof, m, n), SENTINEL, **f64), ksa=torch.full((nprof, m, n), SENTINEL, **f64),
                keep=torch.full((nprof, m), 9, **u8), avk_diag=torch.full((nprof, nblk, nlev), SENTINEL, **f64),
                dfs_block=torch.full((nprof, nblk), SENTINEL, **f64), noise_var=torch.full((nprof, nblk, nlev), SENTINEL, **f64),
                smooth_var=torch.full((nprof, nblk, nlev), SENTINEL, **f64), status=torch.full((nprof,), 9, **u8),
                nobs=torch.full((nprof,), -7, dtype=torch.int32, device="cuda"))


def call_gain(ctx, d, out, case, want=GAIN_KEYS, stream=None, **kw):
    nprof, m, nlev = d["k"][0].shape
    ptr = lambda key: out[key].data_ptr() if key in want else None   # noqa: E731
    args = dict(d_gain=ptr("gain"), d_ksa=ptr("ksa"), d_keep=ptr("keep"), d_avk_diag=ptr("avk_diag"),
                d_dfs_block=ptr("dfs_block"), d_noise_var=ptr("noise_var"), d_smooth_var=ptr("smooth_var"), d_nobs=ptr("nobs"),
                xa_per_profile=case["xa"].ndim == 3, se_full=case["se"].ndim == 2, stream=_cur() if stream is None else stream)
    args.update(kw)
    ctx.oe_gain_device(nprof, nlev, m, [b.data_ptr() for b in d["k"]], d["x"].data_ptr(), d["xa"].data_ptr(),
                       d["sa"].data_ptr(), d["se"].data_ptr(), d["y"].data_ptr(), d["fx"].data_ptr(), ptr("status"), **args)


def run_gain(ctx, case, want=GAIN_KEYS, keep_device=False, **kw):
    """One mwrt_oe_gain_device call on a case of oe_reference.make_case -> dict of NumPy outputs (None where not asked
    for); outputs are pre-filled with a sentinel so an entry the kernel leaves unwritten shows."""
    d = upload(case)
    nprof, m, nlev = d["k"][0].shape
    out = gain_buffers(nprof, len(d["k"]), nlev, m)
    call_gain(ctx, d, out, case, want=want, **kw)
    torch.cuda.synchronize()
    got = {key: (out[key].cpu().numpy() if key in want else None) for key in GAIN_KEYS}
    return (got, d, out) if keep_device else got


def run_product(ctx, product, gain, keep, d, ksa=None, rows=None, nlev=None, **kw):
    """One mwrt_oe_product_device call on device tensors -> NumPy [nprof][count][n].  The result sits between two guard
    rows of the sentinel, which must survive."""
    nprof, m, n = gain.shape
    nblk = len(d["k"])
    nlev = n // nblk if nlev is None else nlev
    r0, rc = (0, 0) if rows is None else rows
    count = rc or n
    flat = torch.full((nprof * count * n + 2 * n,), SENTINEL, dtype=torch.float64, device="cuda")
    args = dict(d_ksa=None if ksa is None else ksa.data_ptr(), d_sa=d["sa"].data_ptr(), row_begin=r0, row_count=rc, stream=_cur())
    args.update(kw)
    ctx.oe_product_device(nprof, nlev, m, product, gain.data_ptr(), keep.data_ptr(), flat[n:].data_ptr(),
                          [b.data_ptr() for b in d["k"]], **args)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:n] == SENTINEL).all() and (host[-n:] == SENTINEL).all(), "the product wrote outside its rows"
    return host[n:-n].reshape(nprof, count, n)


_refs = {}


def case_and_reference(nlev, nblk, m, se_full, xa_pp, nprof=4, products=True):
    """The seeded case and its reference, computed once and shared (never modified).  The full n x n products of the
    2048-state shape are not kept: its tests ask for row windows."""
    key = (nlev, nblk, m, se_full, xa_pp, nprof, products)
    if key not in _refs:
        case = oer.make_case(nlev, nblk, m, nprof=nprof, se_full=se_full, xa_per_profile=xa_pp)
        _refs[key] = (case, ocr.oe_char_reference(**case, products=products))
    return _refs[key]


def check_gain(got, ref, case, label):
    assert got["status"].tolist() == ref["status"].tolist(), label
    assert got["nobs"].tolist() == ref["nobs"].tolist(), label
    assert np.array_equal(got["keep"], ref["keep"]), label
    ok = ref["status"] == 1
    assert ok.any() and np.nanmax(ref["cond"]) <= oer.COND_MAX, (label, ref["cond"])
    err = ocr.char_errors(got, ref, case)
    print(label, err)
    assert all(np.isfinite(got[k][ok]).all() for k in FLOAT_KEYS), label
    assert set(err) == set(FLOAT_KEYS) and all(v <= oer.TOL for v in err.values()), (label, err)
    return err


def _windows(n, nlev):
    """Row windows of the n x n products: everything below n = 2048, two halves there, and beyond it (where a half would be
    [4][1818][3636] doubles) the first 64 rows, the last 64 and 64 rows across the first block seam -- the product kernel's
    tile edges are reached in full at n = 128 and 130."""
    if n < 2048:
        return [None]
    if n == 2048:
        return [(0, n // 2), (n // 2, n // 2)]
    return [(0, 64), (n - 64, 64), (nlev - 32, 64)]


@pytest.mark.parametrize("nlev,nblk,m", oer.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("se_full,xa_pp", COMBOS, ids=COMBO_IDS)
def test_gain_entry_and_chain_against_the_reference(gpu_ctx, nlev, nblk, m, se_full, xa_pp):
    n = nblk * nlev
    case, ref = case_and_reference(nlev, nblk, m, se_full, xa_pp, products=n < 2048)
    got, d, out = run_gain(gpu_ctx, case, keep_device=True)
    label = (nlev, nblk, m, se_full, xa_pp)
    check_gain(got, ref, case, label)
    # the merged entry on the same buffers says the same: status, dfs = sum of dfs_block, post_var = noise + smoothing
    step = run_step(gpu_ctx, case)
    assert step["status"].tolist() == got["status"].tolist()
    bd = ref["bound_diag"].reshape(4, nblk, nlev)
    dsa = np.diag(case["sa"]).reshape(nblk, nlev).max(axis=1)[None, :, None]
    e_dfs = (np.abs(got["dfs_block"].sum(axis=1) - step["dfs"]) / np.maximum(1.0, bd.sum(axis=(1, 2)))).max()
    e_var = (np.abs(got["noise_var"] + got["smooth_var"] - step["post_var"]) / dsa).max()
    print(label, "against the step: dfs", e_dfs, "post_var", e_var)
    assert e_dfs <= oer.TOL and e_var <= oer.TOL
    # the chain: gain -> product on the device buffers, against the reference A and S^
    for rows in _windows(n, nlev):
        r = ref if rows is None else ocr.oe_char_reference(**case, rows=rows)
        chain = dict(avk=run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d, rows=rows),
                     post_cov=run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, out["gain"], out["keep"], d, ksa=out["ksa"], rows=rows))
        err = ocr.char_errors(chain, r, case, rows=rows)
        print(label, "chain", rows, err)
        assert np.isfinite(chain["avk"]).all() and np.isfinite(chain["post_cov"]).all()
        assert set(err) == {"avk", "post_cov"} and all(v <= oer.TOL for v in err.values()), (label, rows, err)


@pytest.mark.parametrize("nlev,nblk,m", oer.SHAPES, ids=SHAPE_IDS)
def test_product_entry_within_the_bound_of_a_length_m_sum(gpu_ctx, nlev, nblk, m):
    n = nblk * nlev
    case, ref = case_and_reference(nlev, nblk, m, False, False, products=False)
    d = upload(case)
    gain, ksa, keep = _dev(ref["gain"]), _dev(ref["ksa"]), _dev(ref["keep"])          # exact inputs: the reference's own
    K = np.concatenate(case["k"], axis=2)
    for rows in _windows(n, nlev):
        r0, rc = (0, n) if rows is None else rows
        a_ref, a_bound = ocr.product_reference(ref["gain"], ref["keep"], K, rows=rows)
        a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, gain, keep, d, rows=rows)
        worst = (np.abs(a - a_ref) / (2 * m * ocr.EPS * a_bound)).max()
        print((nlev, nblk, m), rows, "A: worst error in units of its bound", worst)
        assert (np.abs(a - a_ref) <= 2 * m * ocr.EPS * a_bound).all()
        s_ref, s_bound = ocr.product_reference(ref["gain"], ref["keep"], ref["ksa"], sa=case["sa"], rows=rows)
        s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, gain, keep, d, ksa=ksa, rows=rows)
        bound = 2 * m * ocr.EPS * (np.abs(case["sa"][r0:r0 + rc])[None] + s_bound)
        print((nlev, nblk, m), rows, "S^: worst error in units of its bound", (np.abs(s - s_ref) / bound).max())
        assert (np.abs(s - s_ref) <= bound).all()


def _copy(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else [b.copy() for b in v]) for k, v in case.items()}


def test_product_never_reads_a_dropped_row(gpu_ctx):
    nlev, nblk, m = 65, 2, 98
    case, _ = case_and_reference(nlev, nblk, m, False, False)
    bad = _copy(case)
    bad["y"][1, 41] = np.nan                                  # the row rule drops row 41 of profile 1 ...
    ref = ocr.oe_char_reference(**bad)
    assert ref["keep"][1, 41] == 0 and ref["nobs"].tolist() == [m, m - 1, m, m]
    poisoned = _copy(bad)
    for b in poisoned["k"]:
        b[1, 41] = np.nan                                     # ... and its K and W rows hold NaN when the product runs
    ksa = ref["ksa"].copy()
    ksa[1, 41] = np.nan
    d = upload(poisoned)
    gain, keep = _dev(ref["gain"]), _dev(ref["keep"])
    a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, gain, keep, d)
    s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, gain, keep, d, ksa=_dev(ksa))
    assert np.isfinite(a).all() and np.isfinite(s).all()
    # equal to the product with the row deleted by hand, bit for bit: a skipped row adds an exact zero
    rows = np.arange(m) != 41
    cut = upload(dict(bad, k=[b[:, rows] for b in bad["k"]]))
    a_cut = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, _dev(ref["gain"][:, rows]), _dev(ref["keep"][:, rows]), cut)
    s_cut = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, _dev(ref["gain"][:, rows]), _dev(ref["keep"][:, rows]), cut,
                        ksa=_dev(ref["ksa"][:, rows]))
    assert np.array_equal(a[1], a_cut[1]) and np.array_equal(s[1], s_cut[1])
    K = np.concatenate(bad["k"], axis=2)
    a_ref, a_bound = ocr.product_reference(ref["gain"], ref["keep"], K)
    assert (np.abs(a - a_ref) <= 2 * m * ocr.EPS * a_bound).all()


@pytest.mark.parametrize("nlev,nblk,m", [(65, 2, 98), (33, 1, 17), (64, 2, 15)], ids=["65-2-98", "33-1-17", "64-2-15"])
def test_row_windows_equal_the_full_result_bit_for_bit(gpu_ctx, nlev, nblk, m):
    n = nblk * nlev
    case, ref = case_and_reference(nlev, nblk, m, False, False)
    d = upload(case)
    gain, ksa, keep = _dev(ref["gain"]), _dev(ref["ksa"]), _dev(ref["keep"])
    full_a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, gain, keep, d)
    full_s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, gain, keep, d, ksa=ksa)
    zero = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, gain, keep, d, rows=(0, n))      # all rows, said explicitly
    assert np.array_equal(zero, full_a)
    windows = [(0, 1), (n - 1, 1), (min(nlev - 1, n - 3), 3), (max(0, min(60, n - 9)), min(9, n)), (3, min(70, n - 3))]
    for rows in windows:                                      # first, last, across a block boundary, across a tile edge
        a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, gain, keep, d, rows=rows)
        s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, gain, keep, d, ksa=ksa, rows=rows)
        assert a.shape == (4, rows[1], n)
        assert np.array_equal(a, full_a[:, rows[0]:rows[0] + rows[1]]), rows
        assert np.array_equal(s, full_s[:, rows[0]:rows[0] + rows[1]]), rows


@pytest.mark.parametrize("what", ["y", "fx", "k", "se-diag", "se-full"])
def test_dropped_rows_equal_rows_deleted(gpu_ctx, what):
    nlev, nblk, m, nprof = 65, 2, 98, 4
    base, _ = case_and_reference(nlev, nblk, m, what == "se-full", False)
    clean = run_gain(gpu_ctx, base)
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
        ref = ocr.oe_char_reference(**case)
        shared = what.startswith("se")
        assert ref["nobs"].tolist() == ([m - 1] * nprof if shared else [m, m - 1, m, m])
        got, d, out = run_gain(gpu_ctx, case, keep_device=True)
        check_gain(got, ref, case, (what, row))
        hit = range(nprof) if shared else [1]
        for i in hit:
            assert (got["gain"][i, row] == 0).all() and (got["ksa"][i, row] == 0).all() and got["keep"][i, row] == 0
        # the chain on the device's own buffers: a NaN in K's dropped row must not reach A
        a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d)
        s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, out["gain"], out["keep"], d, ksa=out["ksa"])
        err = ocr.char_errors(dict(avk=a, post_cov=s), ref, case)
        assert np.isfinite(a).all() and np.isfinite(s).all() and all(v <= oer.TOL for v in err.values()), (what, row, err)
        if not shared:                                         # the neighbours never see it: bit for bit
            for i in (0, 2, 3):
                for key in GAIN_KEYS:
                    assert np.array_equal(got[key][i], clean[key][i]), (what, row, i, key)


@pytest.mark.parametrize("pattern", list(oer.SEAM_DROPS))
@pytest.mark.parametrize("what", ["y", "k"])
def test_dropped_rows_at_the_seams_equal_rows_deleted(gpu_ctx, what, pattern):
    """m = 65: row 64 is the only row of the third tile of k_char_gain<3>.  Profile 1 loses the last row of a tile, the
    first of the next, a whole tile (32 rows of zeros in the gain), or every row but 64."""
    (nlev, nblk, m), nprof = oer.SEAM_SHAPE, 4
    dropped = list(oer.SEAM_DROPS[pattern])
    base, _ = case_and_reference(nlev, nblk, m, False, False)
    clean = run_gain(gpu_ctx, base)
    case = oer.drop_rows(base, what, dropped, 1)
    ref = ocr.oe_char_reference(**case)
    assert ref["nobs"].tolist() == [m, m - len(dropped), m, m]
    got, d, out = run_gain(gpu_ctx, case, keep_device=True)
    check_gain(got, ref, case, (what, pattern))
    assert (got["gain"][1, dropped] == 0).all() and (got["ksa"][1, dropped] == 0).all() and (got["keep"][1, dropped] == 0).all()
    # the chain on the device's own buffers: a NaN in K's dropped rows must not reach A
    a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d)
    s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, out["gain"], out["keep"], d, ksa=out["ksa"])
    err = ocr.char_errors(dict(avk=a, post_cov=s), ref, case)
    print((what, pattern), "chain", err)
    alone = oer.one_profile(dict(got, avk=a, post_cov=s), 1)
    print((what, pattern), "profile 1 alone", ocr.char_errors(alone, oer.one_profile(ref, 1), case))
    assert np.isfinite(a).all() and np.isfinite(s).all() and all(v <= oer.TOL for v in err.values()), (what, pattern, err)
    for i in (0, 2, 3):                                        # the neighbours never see it: bit for bit
        for key in GAIN_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (what, pattern, i, key)


def test_status_values_and_untouched_neighbours(gpu_ctx):
    nlev, nblk, m, nprof = 65, 2, 98, 5
    base, _ = case_and_reference(nlev, nblk, m, False, True, nprof=nprof)
    clean = run_gain(gpu_ctx, base)
    case = _copy(base)
    for b in case["k"]:
        b[1] = np.nan                                          # what an invalid profile of the Jacobian call looks like
    case["fx"][1] = np.nan
    case["x"][3, 1, 17] = np.nan
    got, d, out = run_gain(gpu_ctx, case, keep_device=True)
    ref = ocr.oe_char_reference(**case, products=False)
    assert got["status"].tolist() == ref["status"].tolist() == [1, 3, 1, 0, 1]
    assert got["nobs"].tolist() == [m, 0, m, 0, m] and got["keep"].sum(axis=1).tolist() == [m, 0, m, 0, m]
    for key in ("gain", "ksa", "avk_diag", "dfs_block", "noise_var"):
        assert (got[key][1] == 0).all(), key                   # nothing observed: the prior
        assert np.isnan(got[key][3]).all(), key
    assert np.array_equal(got["smooth_var"][1].ravel(), np.diag(case["sa"])) and np.isnan(got["smooth_var"][3]).all()
    for i in (0, 2, 4):
        for key in GAIN_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (i, key)
    # the products of those profiles: keep is 0 throughout, so A = 0 and S^ = Sa (read d_status first, the header says)
    a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d)
    s = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, out["gain"], out["keep"], d, ksa=out["ksa"])
    for i in (1, 3):
        assert (a[i] == 0).all() and np.array_equal(s[i], case["sa"]), i
    # NaN in xa alone is status 0 as well
    case = _copy(base)
    case["xa"][2, 0, 64] = np.inf
    got = run_gain(gpu_ctx, case)
    assert got["status"].tolist() == [1, 1, 0, 1, 1] and np.isnan(got["gain"][2]).all() and (got["keep"][2] == 0).all()
    # an indefinite G: a negative variance larger than K Sa K^T's diagonal
    case = _copy(base)
    case["se"][40] = -1e9
    got = run_gain(gpu_ctx, case)
    assert got["status"].tolist() == [2] * nprof and got["nobs"].tolist() == [m] * nprof and (got["keep"] == 0).all()
    for key in FLOAT_KEYS:
        assert np.isnan(got[key]).all(), key
    assert run_step(gpu_ctx, case)["status"].tolist() == [2] * nprof


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_the_averaging_kernel_is_the_steps_response_to_the_state(gpu_ctx, se_full):
    """x+ is linear in y at fixed K, x and fx: the step at y + K delta minus the step at y is A delta.  Algebra of the
    merged entry alone -- the reference takes no part.  The bar's scale per block is the largest (|gain|^T |K| |delta|)_j
    of the block, with gain from the new path: the sum of absolute values behind (A delta)_j."""
    nlev, nblk, m = 65, 2, 98
    case, _ = case_and_reference(nlev, nblk, m, se_full, False)
    n = nblk * nlev
    got, d, out = run_gain(gpu_ctx, case, keep_device=True)
    a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d)
    rng = np.random.default_rng(17)
    delta = rng.standard_normal((4, nblk, nlev)) * np.array(oer.SIGMA[:nblk])[None, :, None]
    K = np.concatenate(case["k"], axis=2)
    moved = dict(case, y=case["y"] + np.einsum("pik,pk->pi", K, delta.reshape(4, n)))
    x0, x1 = run_step(gpu_ctx, case)["x_new"], run_step(gpu_ctx, moved)["x_new"]
    response = np.einsum("pjk,pk->pj", a, delta.reshape(4, n)).reshape(4, nblk, nlev)
    scale = np.einsum("pij,pik,pk->pj", np.abs(got["gain"]), np.abs(K), np.abs(delta.reshape(4, n))).reshape(4, nblk, nlev)
    err = (np.abs((x1 - x0) - response).max(axis=2) / scale.max(axis=2)).max()
    print("A delta against the step's response:", err)
    assert np.abs(response).max() > 1e-3 and err <= oer.TOL


def test_outputs_do_not_depend_on_the_batch(gpu_ctx):
    nlev, nblk, m = 65, 2, 98
    big = oer.make_case(nlev, nblk, m, nprof=300)

    def everything(case):
        got, d, out = run_gain(gpu_ctx, case, keep_device=True)
        got["avk"] = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d)
        got["post_cov"] = run_product(gpu_ctx, _native.OE_PRODUCT_POST_COV, out["gain"], out["keep"], d, ksa=out["ksa"])
        return got

    got300, again = everything(big), everything(big)
    keys = GAIN_KEYS + ("avk", "post_cov")
    for key in keys:
        assert np.array_equal(got300[key], again[key], equal_nan=True), key
    assert (got300["status"] == 1).all()
    for nprof in (1, 5):
        sub = dict(big, k=[b[:nprof] for b in big["k"]], x=big["x"][:nprof], y=big["y"][:nprof], fx=big["fx"][:nprof])
        got = everything(sub)
        for key in keys:
            assert np.array_equal(got[key], got300[key][:nprof]), (nprof, key)
    j = 299                                                    # the last profile of the large batch as a batch of one
    one = dict(big, k=[b[j:j + 1] for b in big["k"]], x=big["x"][j:j + 1], y=big["y"][j:j + 1], fx=big["fx"][j:j + 1])
    got = everything(one)
    for key in keys:
        assert np.array_equal(got[key][0], got300[key][j]), key


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_optional_outputs_leave_the_gain_unchanged(gpu_ctx, se_full):
    case, _ = case_and_reference(65, 2, 98, se_full, False)
    full = run_gain(gpu_ctx, case)
    for want in (("status", "gain"), ("status", "gain", "keep"), ("status", "gain", "ksa", "nobs"), ("status", "gain", "avk_diag"),
                 ("status", "gain", "noise_var"), ("status", "gain", "smooth_var", "dfs_block"), ("status", "dfs_block"),
                 ("status", "nobs")):
        got = run_gain(gpu_ctx, case, want=want)
        for key in want:
            assert np.array_equal(got[key], full[key]), (want, key)
    # a record that ends after d_gain: everything behind it is absent
    got = run_gain(gpu_ctx, case, want=("status", "gain"), struct_size=_native.MwrtOeChar.d_ksa.offset)
    assert np.array_equal(got["gain"], full["gain"]) and got["status"].tolist() == [1] * 4


def test_short_record_ignores_the_fields_beyond_it(gpu_ctx):
    case, _ = case_and_reference(33, 1, 17, False, False)
    full = run_gain(gpu_ctx, case)
    d = upload(case)
    out = gain_buffers(4, 1, 33, 17)
    rec = _native.MwrtOeChar()
    rec.nblk = 1
    rec.d_k[0] = d["k"][0].data_ptr()
    rec.d_x, rec.d_xa, rec.d_sa, rec.d_se, rec.d_y, rec.d_fx = (d[k].data_ptr() for k in ("x", "xa", "sa", "se", "y", "fx"))
    rec.d_status, rec.d_gain = out["status"].data_ptr(), out["gain"].data_ptr()
    # not addresses: reading them as such would fault; and a reserved2 that would be refused if it were read
    rec.d_ksa = rec.d_keep = rec.d_avk_diag = rec.d_dfs_block = rec.d_noise_var = rec.d_smooth_var = rec.d_nobs = 8
    rec.reserved2 = 5
    # ... whether the record ends at a field boundary or inside d_ksa (a half-copied pointer would be written through)
    for size in (_native.MwrtOeChar.d_ksa.offset, _native.MwrtOeChar.d_ksa.offset + 4):
        rec.struct_size = size
        out["gain"].fill_(SENTINEL)
        out["status"].zero_()
        rc = gpu_ctx._lib.mwrt_oe_gain_device(gpu_ctx._handle, 4, 33, 17, ctypes.byref(rec), _native._stream(_cur()))
        assert rc == 0, gpu_ctx._lib.mwrt_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(out["gain"].cpu().numpy(), full["gain"]) and out["status"].cpu().tolist() == [1] * 4, size
    # a record that ends inside the product's four integers: the ones it ends before are 0 (here: all rows)
    keep = _dev(full["keep"])
    ref_a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], keep, d)
    res = torch.full((4, 33, 33), SENTINEL, dtype=torch.float64, device="cuda")
    rec.d_keep = keep.data_ptr()
    rec.product, rec.row_begin, rec.row_count, rec.reserved2 = 0, 0, 9, 5
    rec.struct_size = _native.MwrtOeChar.row_count.offset + 2          # product and row_begin are read, row_count is not
    rec.d_out = 8
    assert gpu_ctx._lib.mwrt_oe_product_device(gpu_ctx._handle, 4, 33, 17, ctypes.byref(rec), _native._stream(_cur())) == -1  # no d_out
    rec.struct_size = ctypes.sizeof(rec)
    rec.d_out, rec.row_count, rec.reserved2 = res.data_ptr(), 0, 0
    assert gpu_ctx._lib.mwrt_oe_product_device(gpu_ctx._handle, 4, 33, 17, ctypes.byref(rec), _native._stream(_cur())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), ref_a)


def test_argument_refusals(gpu_ctx):
    case = oer.make_case(3, 3, 14, nprof=2)
    d = upload(case)
    out = gain_buffers(2, 3, 3, 14)
    kp = [b.data_ptr() for b in d["k"]]
    base = dict(nprof=2, nlev=3, m=14, d_k=kp, d_x=d["x"].data_ptr(), d_xa=d["xa"].data_ptr(), d_sa=d["sa"].data_ptr(),
                d_se=d["se"].data_ptr(), d_y=d["y"].data_ptr(), d_fx=d["fx"].data_ptr(), d_status=out["status"].data_ptr(),
                d_gain=out["gain"].data_ptr(), d_ksa=out["ksa"].data_ptr(), d_keep=out["keep"].data_ptr(), stream=_cur())

    def refused(fn, args, **change):
        with pytest.raises(MwrtError) as ei:
            fn(**dict(args, **change))
        return ei.value.code, str(ei.value)

    gain = lambda **change: refused(gpu_ctx.oe_gain_device, base, **change)   # noqa: E731
    gpu_ctx.oe_gain_device(**base)                                   # the unchanged call is accepted
    for name in ("d_x", "d_xa", "d_sa", "d_se", "d_y", "d_fx", "d_status"):
        assert gain(**{name: None})[0] == -1, name
    assert gain(d_gain=None, d_ksa=None, d_keep=None)[0] == -1       # no output beside d_status
    gpu_ctx.oe_gain_device(**dict(base, d_gain=None, d_ksa=None))    # one is enough
    assert gain(d_k=[kp[0], None, kp[2]])[0] == -1
    assert gain(d_k=[])[0] == -1 and gain(d_k=[kp[0]] * 5)[0] == -1  # nblk 0 and 5
    assert gain(reserved=1)[0] == -1 and gain(reserved2=1)[0] == -1
    assert gain(nlev=0)[0] == -1 and gain(m=0)[0] == -1 and gain(nprof=-1)[0] == -1
    assert gain(struct_size=23)[0] == -1 and gain(struct_size=0)[0] == -1
    assert gain(struct_size=_native.MwrtOeChar.d_status.offset)[0] == -1             # ends before d_status
    c, text = gain(m=_native.OE_MAX_M + 1)
    assert c == -5 and str(_native.OE_MAX_M) in text
    c, text = gain(nlev=1025)
    assert c == -5 and "1024" in text
    gpu_ctx.oe_gain_device(**dict(base, nprof=0))                    # nothing to do is not an error
    torch.cuda.synchronize()

    res = torch.empty((2, 9, 9), dtype=torch.float64, device="cuda")
    pbase = dict(nprof=2, nlev=3, m=14, product=_native.OE_PRODUCT_POST_COV, d_gain=out["gain"].data_ptr(),
                 d_keep=out["keep"].data_ptr(), d_out=res.data_ptr(), d_k=kp, d_ksa=out["ksa"].data_ptr(),
                 d_sa=d["sa"].data_ptr(), stream=_cur())
    prod = lambda **change: refused(gpu_ctx.oe_product_device, pbase, **change)   # noqa: E731
    gpu_ctx.oe_product_device(**pbase)
    gpu_ctx.oe_product_device(**dict(pbase, d_k=[None] * 3))         # the posterior reads no K
    gpu_ctx.oe_product_device(**dict(pbase, product=_native.OE_PRODUCT_AVK, d_ksa=None, d_sa=None))   # A reads neither W nor Sa
    for name in ("d_gain", "d_keep", "d_out", "d_ksa", "d_sa"):
        assert prod(**{name: None})[0] == -1, name
    assert prod(product=_native.OE_PRODUCT_AVK, d_k=[kp[0], None, kp[2]])[0] == -1
    assert prod(product=2)[0] == -1 and prod(product=-1)[0] == -1
    assert prod(row_begin=-1, row_count=2)[0] == -1 and prod(row_begin=0, row_count=-1)[0] == -1
    assert prod(row_begin=8, row_count=2)[0] == -1 and prod(row_begin=9, row_count=1)[0] == -1   # over n = 9
    assert prod(row_begin=3, row_count=0)[0] == -1                   # "all rows" starts at 0
    gpu_ctx.oe_product_device(**dict(pbase, row_begin=8, row_count=1))
    assert prod(reserved=1)[0] == -1 and prod(reserved2=1)[0] == -1
    assert prod(d_k=[])[0] == -1 and prod(d_k=[None] * 5)[0] == -1
    assert prod(nlev=0)[0] == -1 and prod(m=0)[0] == -1 and prod(nprof=-1)[0] == -1 and prod(struct_size=23)[0] == -1
    c, text = prod(m=_native.OE_MAX_M + 1)
    assert c == -5 and str(_native.OE_MAX_M) in text
    c, text = prod(nlev=1025)
    assert c == -5 and "1024" in text
    gpu_ctx.oe_product_device(**dict(pbase, nprof=0))
    torch.cuda.synchronize()


def test_repeat_call_allocates_nothing_and_orders_on_the_callers_stream(gpu_ctx):
    case, _ = case_and_reference(180, 2, 98, False, False, products=False)
    first, d, out = run_gain(gpu_ctx, case, keep_device=True)
    first_a = run_product(gpu_ctx, _native.OE_PRODUCT_AVK, out["gain"], out["keep"], d)
    res, doubled = torch.empty((4, 360, 360), dtype=torch.float64, device="cuda"), torch.empty((4, 360, 360), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()

    def call(stream):
        call_gain(gpu_ctx, d, out, case, stream=stream)
        gpu_ctx.oe_product_device(4, 180, 98, _native.OE_PRODUCT_AVK, out["gain"].data_ptr(), out["keep"].data_ptr(),
                                  res.data_ptr(), [b.data_ptr() for b in d["k"]], stream=stream)

    with torch.cuda.stream(side):                                    # warm-up of everything this test launches on `side`
        call(side.cuda_stream)
        torch.mul(res, 2.0, out=doubled)
        res.fill_(SENTINEL)
        out["gain"].fill_(SENTINEL)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    call(side.cuda_stream)
    side.synchronize()
    assert torch.cuda.mem_get_info()[0] == before                    # hipMemGetInfo: the calls took and freed nothing
    with torch.cuda.stream(side):
        res.fill_(SENTINEL)
        out["gain"].fill_(SENTINEL)                                  # the product must see the gain of the call before it
        call(side.cuda_stream)
        torch.mul(res, 2.0, out=doubled)                             # consumed on the same stream: ordered behind the kernels
    side.synchronize()                                               # that stream alone, no device-wide wait
    assert np.array_equal(doubled.cpu().numpy(), 2.0 * first_a)
    assert np.array_equal(out["gain"].cpu().numpy(), first["gain"])


# ---- end to end: OneDVar.characterise on the real operator ----
def _retrieval_setup(blocks):
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    nprof, nlev = 3, 40
    P = pr.synthetic_profiles(nprof, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, nlev)).astype(int)           # 40 of the 180 levels, ground to ~12 km
    P = {k: np.ascontiguousarray(v[:, pick]) for k, v in P.items()}
    frq, elev = pr.HATPRO_FRQS, np.array([90.0, 19.2])               # 14 channels x 2 elevations
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    nblk = len(blocks)
    sig = [2.0, 0.1, 0.02][:nblk]                                    # K, rh fraction, g m-3
    lev = np.arange(nlev)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 6.0)
    sa = np.zeros((nblk * nlev, nblk * nlev))
    for b in range(nblk):
        sa[b * nlev:(b + 1) * nlev, b * nlev:(b + 1) * nlev] = sig[b] ** 2 * corr
    se = np.full(frq.size * elev.size, 0.25)
    first = [t, rh] + ([torch.full_like(t, 0.01)] if nblk == 3 else [])
    xa = torch.stack(first, dim=1).contiguous()
    ov = retrieval.OneDVar("R24", frq, elev, _dev(sa), _dev(se), variables=JacVariables.of(humidity="rh"), blocks=blocks, xa=xa)
    bump = np.exp(-((lev - 8.0) / 10.0) ** 2)
    dx = np.stack([1.5 * bump, 0.05 * bump, 0.01 * bump][:nblk])[None] * np.array([0.6, 0.8, 1.0])[:, None, None]
    y, valid = ov.forward(z, p, xa + _dev(dx))
    assert valid.cpu().tolist() == [1] * nprof
    return ov, z, p, y, sa, se


@pytest.mark.parametrize("blocks", [("t", "h"), ("t", "h", "liq")], ids=["t-h", "t-h-liq"])
def test_one_d_var_characterise_on_the_real_operator(gpu_ctx, blocks):
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    ov, z, p, y, sa, se = _retrieval_setup(blocks)
    nprof, nblk, nlev, m = 3, len(blocks), 40, 28
    res = ov.retrieve(z, p, y, max_iter=10, tol=0.05)
    assert (res.status == 1).all()
    ch = ov.characterise(z, p, res.x, y, avk=True, post_cov=True)
    torch.cuda.synchronize()
    # the NumPy reference on the K the device computes at the same state
    zz, t, rh, dl, di = ov.physical(z, p, res.x)
    tb, valid, rows = retrieval._native_k_matrix("R24", zz.contiguous(), p.contiguous(), t, rh, dl, di, ov.frq, ov.elev,
                                                 ov.variables, blocks, _cur())
    torch.cuda.synchronize()
    case = dict(k=[rows[b].cpu().numpy().reshape(nprof, m, nlev) for b in blocks], x=res.x.cpu().numpy(),
                xa=ov.xa.cpu().numpy(), sa=sa, se=se, y=y.cpu().numpy().reshape(nprof, m), fx=tb.cpu().numpy().reshape(nprof, m))
    ref = ocr.oe_char_reference(**case)
    got = {k: getattr(ch, k).cpu().numpy() for k in ("gain", "keep", "avk_diag", "dfs_block", "noise_var", "smooth_var",
                                                     "status", "nobs", "avk", "post_cov")}
    print(blocks, "cond_2(G)", ref["cond"])
    assert ref["status"].tolist() == got["status"].tolist() == [1] * nprof and got["nobs"].tolist() == [m] * nprof
    assert np.nanmax(ref["cond"]) <= oer.COND_MAX
    err = ocr.char_errors(got, ref, case)
    print(blocks, err)
    assert set(err) == {"gain", "avk_diag", "dfs_block", "noise_var", "smooth_var", "avk", "post_cov"}
    assert all(v <= oer.TOL for v in err.values()), err
    # retrieve's diagnostics are those of its last step, taken at the state before it: the step at the result instead
    dsa = np.diag(sa).reshape(nblk, nlev).max(axis=1)[None, :, None]
    bsum = np.maximum(1.0, ref["bound_diag"].sum(axis=1))
    _, d = ov.step(z, p, res.x, y)
    assert (np.abs(got["dfs_block"].sum(axis=1) - d["dfs"].cpu().numpy()) / bsum).max() <= oer.TOL
    diag = np.diagonal(got["post_cov"], axis1=1, axis2=2).reshape(nprof, nblk, nlev)
    assert (np.abs(diag - d["post_var"].cpu().numpy()) / dsa).max() <= oer.TOL
    assert (got["dfs_block"] > 0).all() and (got["dfs_block"].sum(axis=1) < m).all()
    # retrieve_lm's Retrieval holds the undamped diagnostics at its own result: dfs and post_var as they are returned
    lm = ov.retrieve_lm(z, p, y, max_iter=20, tol=0.05)
    cl = ov.characterise(z, p, lm.x, y, post_cov=True)
    torch.cuda.synchronize()
    assert (lm.status == 1).all() and (cl.status == 1).all()
    e_dfs = (np.abs(cl.dfs_block.sum(dim=1).cpu().numpy() - lm.dfs.cpu().numpy()) / bsum).max()
    diag = torch.diagonal(cl.post_cov, dim1=1, dim2=2).reshape(nprof, nblk, nlev)
    e_var = (np.abs((diag - lm.post_var).cpu().numpy()) / dsa).max()
    e_sum = (np.abs((cl.noise_var + cl.smooth_var - lm.post_var).cpu().numpy()) / dsa).max()
    print(blocks, "against Retrieval: dfs", e_dfs, "post_var", e_var, e_sum)
    assert e_dfs <= oer.TOL and e_var <= oer.TOL and e_sum <= oer.TOL
