"""mwrt_obs_whiten_device and mwrt_obs_whiten_apply_device (include/mwrt.h) on the GPU against
tests/whiten_reference.py.

The bar of K~, y~, F~ and the un-whitened gain, every element, no mask and no floor: 1e-9 of the column's largest reference
entry -- c m eps cond_2(Se_p) with c = 64, m <= 140 and cond_2 <= 1e2 (asserted on the reference) is 2e-10, rounded up.
L L^T reproduces the kept Se_p to 64 m eps max |Se_p|.  The largest errors met are printed, and written to the file
MWRT_WHITEN_ERRORS_JSON names when it is set (profiles/whiten_errors.json is such a run)."""
import json
import os

import numpy as np
import pytest

import oe_char_reference as ocr
import oe_reference as oer
import whiten_reference as whr
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -7.0
_cases = {}
_worst = {}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


def case(shape, se_full=True):
    """The seeded inputs of a shape and their reference, made once and left alone."""
    key = (shape, se_full)
    if key not in _cases:
        c = whr.make_case(shape, se_full=se_full)
        c["wref"] = whr.whiten_reference(c["k"], c["se_p"], c["y"], c["fx"])
        _cases[key] = c
    return _cases[key]


def note(key, value):
    _worst[key] = max(_worst.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def errors_file():
    """Prints the largest errors met; with MWRT_WHITEN_ERRORS_JSON set to a path, writes them there as well -- how
    profiles/whiten_errors.json is made (a run of the whole module, so that every family is in it)."""
    yield
    if _worst:
        print("\nlargest error per family, in units of its bar's scale:\n" + "\n".join("  %-16s %.3e" % kv for kv in sorted(_worst.items())))
        path = os.environ.get("MWRT_WHITEN_ERRORS_JSON")
        if path:
            with open(path, "w") as f:
                json.dump({"unit": "largest error met, in units of the bar's scale (bar 1e-9; llt: 64 m eps max|Se_p|)",
                           "errors": dict(sorted(_worst.items()))}, f, indent=1)
                f.write("\n")


def whiten(ctx, k, se, y, fx, want_y=True, want_fx=True, want_k=None, **kw):
    """One combined call on NumPy inputs -> dict of NumPy outputs; every output is pre-filled with a sentinel so an element
    the kernels leave unwritten shows.  ``want_k``: which blocks to ask for (default: all)."""
    nprof, m = y.shape
    nlev = kw.pop("nlev", k[0].shape[2] if k else 1)
    want_k = [True] * len(k) if want_k is None else want_k
    d_k = [_dev(b) for b in k]
    d_se, d_y, d_fx = _dev(se), _dev(y), _dev(fx)
    f64 = dict(dtype=torch.float64, device="cuda")
    u8 = dict(dtype=torch.uint8, device="cuda")
    out = dict(l=torch.full((nprof, m * (m + 1) // 2), SENTINEL, **f64), keep=torch.full((nprof, m), 9, **u8),
               status=torch.full((nprof,), 9, **u8), y_out=torch.full((nprof, m), SENTINEL, **f64),
               fx_out=torch.full((nprof, m), SENTINEL, **f64),
               k_out=[torch.full((nprof, m, nlev), SENTINEL, **f64) for _ in k])
    ctx.obs_whiten_device(nprof, nlev, m, d_se.data_ptr(), d_y.data_ptr(), d_fx.data_ptr(), [b.data_ptr() for b in d_k],
                          out["l"].data_ptr(), out["keep"].data_ptr(), out["status"].data_ptr(),
                          d_y_out=out["y_out"].data_ptr() if want_y else None,
                          d_fx_out=out["fx_out"].data_ptr() if want_fx else None,
                          d_k_out=[o.data_ptr() if w else None for o, w in zip(out["k_out"], want_k)],
                          se_full=np.ndim(se) == 3, stream=_cur(), **kw)
    torch.cuda.synchronize()
    return {key: ([o.cpu().numpy() for o in v] if isinstance(v, list) else v.cpu().numpy()) for key, v in out.items()}


def apply(ctx, l, keep, mode, vecs=(), blocks=(), **kw):
    """One apply call with a stored factor -> (list of vectors, list of blocks) as NumPy."""
    nprof, m = keep.shape
    nlev = blocks[0].shape[2] if len(blocks) else kw.pop("nlev", 1)
    kw.pop("nlev", None)
    d_l, d_keep = _dev(l), _dev(keep)
    d_v = [_dev(v) for v in vecs] + [None, None]
    o_v = [torch.full(v.shape, SENTINEL, dtype=torch.float64, device="cuda") for v in vecs] + [None, None]
    d_b = [_dev(b) for b in blocks]
    o_b = [torch.full(b.shape, SENTINEL, dtype=torch.float64, device="cuda") for b in blocks]
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    ctx.obs_whiten_apply_device(nprof, nlev, m, d_l.data_ptr(), d_keep.data_ptr(), mode=mode, d_y=ptr(d_v[0]),
                                d_y_out=ptr(o_v[0]), d_fx=ptr(d_v[1]), d_fx_out=ptr(o_v[1]),
                                d_k_in=[b.data_ptr() for b in d_b], d_k_out=[o.data_ptr() for o in o_b], stream=_cur(), **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in o_v[:len(vecs)]], [o.cpu().numpy() for o in o_b]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64) if np.asarray(a).dtype == np.float64 else a,
                          np.asarray(b).view(np.uint64) if np.asarray(b).dtype == np.float64 else b)


def same_outputs(a, b, rows=slice(None)):
    return (all(same_bits(a[key][rows], b[key][rows]) for key in ("l", "keep", "status", "y_out", "fx_out"))
            and all(same_bits(x[rows], y[rows]) for x, y in zip(a["k_out"], b["k_out"])))


def check_against_reference(got, ref, se, label):
    """keep, status and the pattern of NaN and 0.0 exactly; the numbers at the bar."""
    nprof, m = ref["keep"].shape
    assert np.array_equal(got["keep"], ref["keep"]) and np.array_equal(got["status"], ref["status"]), label
    worst = dict(llt=0.0, l=0.0)
    for p in range(nprof):
        if ref["status"][p] == 2:
            assert np.isnan(got["l"][p]).all(), label
            continue
        lfull = whr.tri_unpack(got["l"][p], m)
        kept = ref["keep"][p] != 0
        drop = np.flatnonzero(~kept)
        assert np.array_equal(lfull[drop], np.eye(m)[drop]) and not lfull[np.ix_(kept, ~kept)].any(), label
        if kept.any():
            s = ref["se_kept"][p]
            lk = lfull[np.ix_(kept, kept)]
            worst["llt"] = max(worst["llt"], np.abs(lk @ lk.T - s).max() / (64 * m * whr.EPS * np.abs(s).max()))
            worst["l"] = max(worst["l"], np.abs(got["l"][p] - ref["l"][p]).max() / np.abs(ref["l"][p]).max())
    worst["y"] = whr.column_errors(got["y_out"], ref["y_out"])
    worst["fx"] = whr.column_errors(got["fx_out"], ref["fx_out"])
    worst["k"] = max([whr.column_errors(g, r) for g, r in zip(got["k_out"], ref["k_out"])], default=0.0)
    for g, r in zip(got["k_out"], ref["k_out"]):
        assert (g[r == 0.0] == 0.0).all() and not np.signbit(g[(r == 0.0) & ~ref["keep"].astype(bool)[:, :, None]]).any(), label
    print(label, "largest errors in units of their bars' scales:", worst)
    for key, v in worst.items():
        note(key, v)
    assert worst["llt"] <= 1.0 and max(worst["l"], worst["y"], worst["fx"], worst["k"]) <= whr.BAR, (label, worst)


@pytest.mark.parametrize("se_full", (True, False), ids=("full", "variances"))
@pytest.mark.parametrize("shape", whr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_entries_against_the_reference(gpu_ctx, shape, se_full):
    nlev, nblk, m = shape
    c = case(shape, se_full)
    ref = c["wref"]
    got = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"], nlev=nlev)
    check_against_reference(got, ref, c["se_p"], (shape, se_full))
    # determinism: the same call again; the second profile alone; fewer outputs asked for
    assert same_outputs(whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"], nlev=nlev), got)
    alone = whiten(gpu_ctx, [b[1:2] for b in c["k"]], c["se_p"][1:2], c["y"][1:2], c["fx"][1:2], nlev=nlev)
    assert all(same_bits(alone[key][0], got[key][1]) for key in ("l", "keep", "status", "y_out", "fx_out"))
    assert all(same_bits(a[0], g[1]) for a, g in zip(alone["k_out"], got["k_out"]))
    want_k = [b == nblk - 1 for b in range(nblk)]
    few = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"], want_y=False, want_k=want_k, nlev=nlev)
    assert (few["y_out"] == SENTINEL).all() and all((o == SENTINEL).all() for o in few["k_out"][:-1])
    assert all(same_bits(few[key], got[key]) for key in ("l", "keep", "status", "fx_out"))
    assert nblk == 0 or same_bits(few["k_out"][-1], got["k_out"][-1])
    only_factor = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"], want_y=False, want_fx=False, want_k=[False] * nblk, nlev=nlev)
    assert all(same_bits(only_factor[key], got[key]) for key in ("l", "keep", "status"))
    # the stored factor applied: bit for bit the combined call
    vecs, blocks = apply(gpu_ctx, got["l"], got["keep"], 0, vecs=(c["y"], c["fx"]), blocks=c["k"], nlev=nlev)
    assert same_bits(vecs[0], got["y_out"]) and same_bits(vecs[1], got["fx_out"])
    assert all(same_bits(b, g) for b, g in zip(blocks, got["k_out"]))
    # ... one vector alone, and the transposed direction on a gain-like block [nprof][m][ncol] and a vector
    vecs, _ = apply(gpu_ctx, got["l"], got["keep"], 0, vecs=(c["fx"],), nlev=nlev)
    assert same_bits(vecs[0], got["fx_out"])                             # in the other vector's lane
    rng = np.random.default_rng([5, nlev, nblk, m])
    gain = rng.standard_normal((c["y"].shape[0], m, max(nlev, 1)))
    vecs, blocks = apply(gpu_ctx, got["l"], got["keep"], 1, vecs=(c["y"],), blocks=(gain,))
    err = dict(gain=whr.column_errors(blocks[0], whr.apply_reference(ref["l"], ref["keep"], gain, 1)),
               y_t=whr.column_errors(vecs[0], whr.apply_reference(ref["l"], ref["keep"], c["y"], 1)))
    print(shape, "transposed:", err)
    note("gain", err["gain"])
    assert max(err.values()) <= whr.BAR, (shape, err)
    _, again = apply(gpu_ctx, got["l"], got["keep"], 1, blocks=(gain[:, :, :1].copy(),))
    assert same_bits(again[0], blocks[0][:, :, :1])                      # a column beside fewer others


def make_drop(c, way, rows, prof):
    """A copy of the case in which profile ``prof`` loses ``rows``: NaN in y, in one K element, or in one Se element."""
    bad = dict(c)
    bad["k"], bad["y"], bad["se_p"] = [b.copy() for b in c["k"]], c["y"].copy(), c["se_p"].copy()
    nblk, nlev, m = len(c["k"]), c["k"][0].shape[2], c["y"].shape[1]
    for row in rows:
        if way == "y":
            bad["y"][prof, row] = np.nan
        elif way == "k":
            bad["k"][row % nblk][prof, row, (7 * row) % nlev] = np.nan
        elif bad["se_p"].ndim == 3:
            bad["se_p"][prof, row, (5 * row) % m] = np.nan
        else:
            bad["se_p"][prof, row] = np.nan
    return bad


@pytest.mark.parametrize("se_full", (True, False), ids=("full", "variances"))
@pytest.mark.parametrize("way", ("y", "k", "se"))
@pytest.mark.parametrize("name", sorted(whr.SEAM_DROPS))
def test_dropped_rows(gpu_ctx, name, way, se_full):
    """keep is the reference's; a dropped row is NaN in the vectors and exact 0.0 in K; no other profile changes a bit, nor
    does a row before the first dropped one, nor -- with variances, where the rows do not mix -- any other row at all.  With
    a full Se_p the rows behind a dropped one are those of another factor and are held against the reference."""
    rows, prof = whr.SEAM_DROPS[name], 1
    c = case(whr.SEAM_SHAPE, se_full)
    clean = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"])
    bad = make_drop(c, way, rows, prof)
    got = whiten(gpu_ctx, bad["k"], bad["se_p"], bad["y"], bad["fx"])
    ref = whr.whiten_reference(bad["k"], bad["se_p"], bad["y"], bad["fx"])
    check_against_reference(got, ref, bad["se_p"], (name, way, se_full))
    assert got["status"][prof] == (3 if name == "all" else 1) and not got["keep"][prof][list(rows)].any()
    assert got["keep"][prof].sum() == 65 - len(rows)
    assert np.isnan(got["y_out"][prof, list(rows)]).all() and np.isnan(got["fx_out"][prof, list(rows)]).all()
    for o in got["k_out"]:
        z = o[prof, list(rows)]
        assert (z == 0.0).all() and not np.signbit(z).any()
    others = [p for p in range(c["y"].shape[0]) if p != prof]
    assert same_outputs(got, clean, others)
    untouched = np.arange(65) < min(rows) if se_full else ~np.isin(np.arange(65), rows)
    for key in ("y_out", "fx_out"):
        assert same_bits(got[key][prof, untouched], clean[key][prof, untouched])
    for g, cl in zip(got["k_out"], clean["k_out"]):
        assert same_bits(g[prof, untouched], cl[prof, untouched])


def test_an_indefinite_se_is_status_2_for_its_profile_alone(gpu_ctx):
    for shape in ((3, 3, 5), (65, 2, 65)):
        c = case(shape)
        clean = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"])
        se = c["se_p"].copy()
        se[2] = -se[2]                                                   # the first pivot fails
        se[0, -1, -1] = 0.0 if shape[2] > 1 else se[0, -1, -1]           # ... and in profile 0 the last one
        got = whiten(gpu_ctx, c["k"], se, c["y"], c["fx"])
        assert list(got["status"]) == [2, 1, 2, 1]
        for p in (0, 2):
            assert not got["keep"][p].any() and np.isnan(got["l"][p]).all()
            assert np.isnan(got["y_out"][p]).all() and np.isnan(got["fx_out"][p]).all()
            assert all(np.isnan(o[p]).all() for o in got["k_out"])
        assert same_outputs(got, clean, [1, 3])
        # the stored NaN factor applied: NaN in every output, in both directions
        for mode in (0, 1):
            vecs, blocks = apply(gpu_ctx, got["l"], got["keep"], mode, vecs=(c["y"],), blocks=c["k"])
            assert np.isnan(vecs[0][[0, 2]]).all() and all(np.isnan(b[[0, 2]]).all() for b in blocks)
            assert np.isfinite(vecs[0][[1, 3]]).all()


def test_a_non_finite_trial_value_stays_behind_its_row(gpu_ctx):
    """mode 0 on F(x_trial): rows of the linearisation, so a NaN in a kept row is not dropped -- it reaches that row and the
    kept rows after it, and no row before it."""
    c = case(whr.SEAM_SHAPE)
    got = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"])
    f = c["fx"].copy()
    f[1, 37] = np.nan
    f[2, 64] = np.inf
    vecs, _ = apply(gpu_ctx, got["l"], got["keep"], 0, vecs=(f,))
    assert same_bits(vecs[0][[0, 3]], got["fx_out"][[0, 3]])
    assert same_bits(vecs[0][1, :37], got["fx_out"][1, :37]) and not np.isfinite(vecs[0][1, 37:]).any()
    assert same_bits(vecs[0][2, :64], got["fx_out"][2, :64]) and not np.isfinite(vecs[0][2, 64])


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    nlev, nblk, m, nprof = 5, 2, 6, 2
    c = whr.make_case((nlev, nblk, m), nprof=nprof)
    t = dict(se=_dev(c["se_p"]), y=_dev(c["y"]), fx=_dev(c["fx"]), k=[_dev(b) for b in c["k"]])
    f64 = dict(dtype=torch.float64, device="cuda")
    o = dict(l=torch.full((nprof, m * (m + 1) // 2), SENTINEL, **f64), keep=torch.full((nprof, m), 9, dtype=torch.uint8, device="cuda"),
             status=torch.full((nprof,), 9, dtype=torch.uint8, device="cuda"), y=torch.full((nprof, m), SENTINEL, **f64),
             fx=torch.full((nprof, m), SENTINEL, **f64), k=[torch.full((nprof, m, nlev), SENTINEL, **f64) for _ in range(nblk)])
    P = lambda v: v.data_ptr()   # noqa: E731

    def w(nprof=nprof, nlev=nlev, m=m, **kw):
        a = dict(d_se=P(t["se"]), d_y=P(t["y"]), d_fx=P(t["fx"]), d_k_in=[P(b) for b in t["k"]], d_l=P(o["l"]),
                 d_keep=P(o["keep"]), d_status=P(o["status"]), d_y_out=P(o["y"]), d_fx_out=P(o["fx"]),
                 d_k_out=[P(b) for b in o["k"]], se_full=True, stream=_cur())
        a.update(kw)
        gpu_ctx.obs_whiten_device(nprof, nlev, m, **a)

    def ap(nprof=nprof, nlev=nlev, m=m, **kw):
        a = dict(d_l=P(o["l"]), d_keep=P(o["keep"]), mode=0, d_y=P(t["y"]), d_y_out=P(o["y"]), d_fx=P(t["fx"]),
                 d_fx_out=P(o["fx"]), d_k_in=[P(b) for b in t["k"]], d_k_out=[P(b) for b in o["k"]], stream=_cur())
        a.update(kw)
        gpu_ctx.obs_whiten_apply_device(nprof, nlev, m, **a)

    invalid = [lambda: w(d_se=None), lambda: w(d_y=None), lambda: w(d_fx=None), lambda: w(d_l=None), lambda: w(d_keep=None),
               lambda: w(d_status=None), lambda: w(d_k_in=[P(t["k"][0]), None]), lambda: w(nblk=5), lambda: w(nblk=-1),
               lambda: w(m=0), lambda: w(nlev=0), lambda: w(nprof=-1), lambda: w(reserved=1), lambda: w(mode=1),
               lambda: w(struct_size=16), lambda: w(d_y_out=P(t["y"])), lambda: w(d_k_out=[P(t["k"][0]), P(o["k"][1])]),
               lambda: w(d_fx_out=P(t["fx"])),
               lambda: ap(d_l=None), lambda: ap(d_keep=None), lambda: ap(d_y_out=None), lambda: ap(d_y=None),
               lambda: ap(d_fx=None), lambda: ap(d_k_out=[P(o["k"][0]), None]), lambda: ap(d_k_in=[None, P(t["k"][1])]),
               lambda: ap(nblk=5), lambda: ap(mode=2), lambda: ap(mode=-1), lambda: ap(reserved=1), lambda: ap(struct_size=23),
               lambda: ap(m=0), lambda: ap(nlev=0), lambda: ap(nprof=-1), lambda: ap(d_y_out=P(t["y"])),
               lambda: ap(d_k_out=[P(t["k"][0]), P(o["k"][1])]),
               lambda: ap(d_y=None, d_y_out=None, d_fx=None, d_fx_out=None, d_k_in=[], d_k_out=[])]
    unsupported = [lambda: w(m=141), lambda: w(nlev=1025), lambda: w(nprof=2 ** 31), lambda: ap(m=141), lambda: ap(nlev=1025),
                   lambda: ap(nprof=2 ** 31 // 3 + 1)]
    for code, calls in ((-1, invalid), (-5, unsupported)):
        for i, call in enumerate(calls):
            with pytest.raises(MwrtError) as ei:
                call()
            assert ei.value.code == code, (code, i, ei.value)
    w(nprof=0)                                                           # MWRT_OK, and nothing is launched
    ap(nprof=0)
    torch.cuda.synchronize()
    assert all((v == SENTINEL).all() for v in (o["l"], o["y"], o["fx"], *o["k"])) and (o["keep"] == 9).all() and (o["status"] == 9).all()
    # a record that ends before the optional outputs: they are NULL, the rest is done
    import ctypes
    from mwr_fast_forward_operators_and_lbls_amd._native import MwrtObsWhiten
    w(struct_size=MwrtObsWhiten.d_y_out.offset + 4)
    torch.cuda.synchronize()
    assert (o["y"] == SENTINEL).all() and (o["k"][0] == SENTINEL).all() and (o["status"] == 1).all()
    assert ctypes.sizeof(MwrtObsWhiten) == 152


def test_a_repeat_call_allocates_nothing(gpu_ctx):
    shape = (180, 3, 140)                                                # both kernels beyond the default LDS limit
    c = case(shape)
    whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"])
    d = [_dev(b) for b in c["k"]] + [_dev(c[key]) for key in ("se_p", "y", "fx")]
    nprof, m, nlev = c["y"].shape[0], shape[2], shape[0]
    l = torch.empty((nprof, m * (m + 1) // 2), dtype=torch.float64, device="cuda")
    keep = torch.empty((nprof, m), dtype=torch.uint8, device="cuda")
    status = torch.empty((nprof,), dtype=torch.uint8, device="cuda")
    outs = [torch.empty_like(b) for b in d[:3]]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        gpu_ctx.obs_whiten_device(nprof, nlev, m, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), [b.data_ptr() for b in d[:3]],
                                  l.data_ptr(), keep.data_ptr(), status.data_ptr(), d_k_out=[b.data_ptr() for b in outs],
                                  se_full=True, stream=_cur())
        gpu_ctx.obs_whiten_apply_device(nprof, nlev, m, l.data_ptr(), keep.data_ptr(), mode=1, d_k_in=[outs[0].data_ptr()],
                                        d_k_out=[outs[1].data_ptr()], stream=_cur())
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0 and (status == 1).all()


E2E_SHAPES = [(3, 3, 5), (65, 2, 65), (180, 2, 98)]


@pytest.mark.parametrize("shape", E2E_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whiten_then_the_step_and_the_gain_on_the_device(gpu_ctx, shape):
    """Whiten, then mwrt_oe_step_device with se = ones against oe_step_reference per profile with its own Se_p, at TOL; whiten,
    the gain entry, un-whiten against oe_char_reference at that family's bar (TOL of the block's largest entry).  Profile 1
    loses two rows."""
    nlev, nblk, m = shape
    c = dict(case(shape))
    c["y"] = c["y"].copy()
    c["y"][1, [0, m - 1]] = np.nan
    nprof, n = c["y"].shape[0], nblk * nlev
    got = whiten(gpu_ctx, c["k"], c["se_p"], c["y"], c["fx"])
    f64 = dict(dtype=torch.float64, device="cuda")
    d_k = [_dev(b) for b in got["k_out"]]
    d_x, d_xa, d_sa, d_one = _dev(c["x"]), _dev(c["xa"]), _dev(c["sa"]), torch.ones(m, **f64)
    d_y, d_fx = _dev(got["y_out"]), _dev(got["fx_out"])
    x_new, post = torch.empty((nprof, nblk, nlev), **f64), torch.empty((nprof, nblk, nlev), **f64)
    chi2, dfs = torch.empty(nprof, **f64), torch.empty(nprof, **f64)
    status = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    nobs = torch.empty(nprof, dtype=torch.int32, device="cuda")
    args = (nprof, nlev, m, [b.data_ptr() for b in d_k], d_x.data_ptr(), d_xa.data_ptr(), d_sa.data_ptr(), d_one.data_ptr(),
            d_y.data_ptr(), d_fx.data_ptr())
    gpu_ctx.oe_step_device(*args, x_new.data_ptr(), status.data_ptr(), d_chi2=chi2.data_ptr(), d_dfs=dfs.data_ptr(),
                           d_post_var=post.data_ptr(), d_nobs=nobs.data_ptr(), stream=_cur())
    gain = torch.empty((nprof, m, n), **f64)
    gstatus = torch.empty(nprof, dtype=torch.uint8, device="cuda")
    noise = torch.empty((nprof, nblk, nlev), **f64)
    gpu_ctx.oe_gain_device(*args, gstatus.data_ptr(), d_gain=gain.data_ptr(), d_noise_var=noise.data_ptr(), stream=_cur())
    phys = torch.empty_like(gain)
    d_l, d_keep = _dev(got["l"]), _dev(got["keep"])
    gpu_ctx.obs_whiten_apply_device(nprof, n, m, d_l.data_ptr(), d_keep.data_ptr(), mode=1, d_k_in=[gain.data_ptr()],
                                    d_k_out=[phys.data_ptr()], stream=_cur())
    torch.cuda.synchronize()
    step = dict(x_new=x_new.cpu().numpy(), post_var=post.cpu().numpy(), chi2=chi2.cpu().numpy(), dfs=dfs.cpu().numpy())
    worst = {}
    for p in range(nprof):
        own = whr.own_case(c, p)
        args_own = {key: own[key] for key in ("k", "x", "xa", "sa", "se", "y", "fx")}
        ref = oer.oe_step_reference(**args_own)
        assert ref["status"][0] == 1 == status[p].item() == gstatus[p].item() and ref["nobs"][0] == nobs[p].item()
        assert ref["cond"][0] <= oer.COND_MAX
        err = oer.block_errors(oer.one_profile(step, p), ref, own)
        cref = ocr.oe_char_reference(**args_own, products=False)
        err.update(ocr.char_errors(dict(gain=phys[p:p + 1].cpu().numpy(), noise_var=noise[p:p + 1].cpu().numpy()), cref, own))
        for key, v in err.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(shape, "largest errors in units of their scales:", worst)
    for key, v in worst.items():
        note("e2e_" + key, v)
    assert max(worst.values()) <= oer.TOL, (shape, worst)
    dropped = phys[1, [0, m - 1]].cpu().numpy()
    assert (dropped == 0.0).all()
