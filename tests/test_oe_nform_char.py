"""mwrt_oe_nform_char_device and mwrt_oe_nform_gain_device (include/mwrt.h) on the GPU, driven behind
mwrt_oe_nform_prepare_device, against tests/nform_char_reference.py.  The bar is nform_reference.TOL = 64 * 128 * eps * 1e4
(Cholesky and its solves on the Jacobi-scaled C at cond <= COND_MAX, asserted per case and profile) in the units of
``char_errors``; no mask, no floor.  Shapes: nform_char_reference.SHAPES, held against the plans as built by
test_nform_char_kernel_resources.py::test_the_shapes_keep_both_sides_of_every_edge.  Every case has 4 profiles."""
import numpy as np
import pytest

import nform_char_reference as ncr
import nform_reference as nfr
import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nform_char_device import CHAR_KEYS, OPTIONAL, CharDev, _dev, as_reference, reference, seeded  # noqa: E402

FLOAT_KEYS = ("c_post_cov", "avk", "avk_diag", "noise_var", "smooth_var", "dfs_block", "gain")
ALL_KEYS = CHAR_KEYS + ("gain",)


def check(got, ref, case, label):
    assert got["c_status"].tolist() == ref["status"].tolist(), label
    ok = ref["status"] == 1
    if ok.any():
        assert ref["cond"][ok].max() <= nfr.COND_MAX, (label, ref["cond"])
    err = ncr.char_errors(as_reference(got), ref, case)
    print(label, err)
    for key in FLOAT_KEYS:
        assert np.isfinite(got[key][ok]).all(), (label, key)
    if ok.any():
        assert max(err.values()) <= nfr.TOL, (label, err)
    bad = (ref["status"] == 0) | (ref["status"] == 2)
    for key in FLOAT_KEYS:
        assert np.isnan(got[key][bad]).all(), (label, key)
    for i in np.flatnonzero(ok):
        assert np.array_equal(got["c_post_cov"][i], got["c_post_cov"][i].T), label
        assert (got["gain"][i][ref["keep"][i] == 0] == 0.0).all(), label
        np.testing.assert_array_equal(np.diagonal(got["avk"][i]), got["avk_diag"][i].reshape(-1))
        np.testing.assert_array_equal(got["smooth_var"][i].reshape(-1), np.diag(got["c_post_cov"][i]) - got["noise_var"][i].reshape(-1))


@pytest.mark.parametrize("nlev,nblk,m", ncr.SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in ncr.SHAPES])
@pytest.mark.parametrize("se_pp,xa_pp", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["shared-shared", "seperprofile-shared", "shared-xaperprofile", "perprofile-perprofile"])
def test_char_and_gain_against_the_reference(gpu_ctx, nlev, nblk, m, se_pp, xa_pp):
    nprof = 4
    case, ref = seeded(nlev, nblk, m, se_pp, xa_pp, nprof)
    label = (nlev, nblk, m, se_pp, xa_pp)
    assert ref["status"].tolist() == [1] * nprof
    d = CharDev(case)
    got = d.characterise(gpu_ctx)
    check(got, ref, case, label)
    # the solve's C^-1 and status serve the gain entry too; the two inverses agree to the bar
    gpu_ctx.oe_nform_solve_device(**d.solve_args())
    d.out["gain"].fill_(-7.0)
    gpu_ctx.oe_nform_gain_device(**d.gain_args(from_solve=True))
    torch.cuda.synchronize()
    again = d.host()
    err = ncr.char_errors(dict(gain=again["gain"], post_cov=again["post_cov"]), ref, case)
    print(label, "from the solve", err)
    assert max(err.values()) <= nfr.TOL, (label, err)


def test_dropped_rows_have_no_gain_and_reach_nothing_else(gpu_ctx):
    """A NaN K row, a NaN y and a NaN variance each drop their row in profile 1: rows at a row-tile seam (127 | 128), the
    first and the last."""
    nlev, nblk, m, nprof = 33, 1, 141, 4
    base = seeded(nlev, nblk, m, True, False, nprof)[0]
    clean = CharDev(base).characterise(gpu_ctx)
    case = oer.copy_case(base)
    case["k"][0][1, 127, 5] = np.nan
    case["k"][0][1, 0, :] = np.nan
    case["y"][1, 128] = np.nan
    case["se"][1, m - 1] = np.nan
    ref = reference(case)
    assert ref["nobs"].tolist() == [m, m - 4, m, m] and ref["status"].tolist() == [1] * nprof
    got = CharDev(case).characterise(gpu_ctx)
    check(got, ref, case, "dropped rows")
    assert got["keep"][1].sum() == m - 4 and (got["gain"][1][[0, 127, 128, m - 1]] == 0.0).all()
    for i in (0, 2, 3):                                                  # the neighbours never see it: bit for bit
        for key in ALL_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (i, key)


def test_status_values_beside_a_good_profile(gpu_ctx):
    nlev, nblk, m, nprof = 16, 2, 20, 6
    base = nfr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=True, xa_per_profile=True)
    clean = CharDev(base).characterise(gpu_ctx)
    case = oer.copy_case(base)
    case["x"][1, 0, 3] = np.nan                                          # lin_status 0
    case["se"][2, 7] = -0.25                                             # lin_status 2
    for b in case["k"]:
        b[3] = np.nan                                                    # lin_status 3
    ref = reference(case)
    assert ref["lin_status"].tolist() == [1, 0, 2, 3, 1, 1] and ref["status"].tolist() == [1, 0, 2, 3, 1, 1]
    d = CharDev(case)
    got = d.characterise(gpu_ctx)
    check(got, ref, case, "statuses")
    for key in ("avk", "avk_diag", "noise_var", "dfs_block", "gain"):
        assert (got[key][3] == 0.0).all(), key
    scale = np.abs(ref["post_cov"][3]).max()
    assert np.abs(got["c_post_cov"][3] - ref["post_cov"][3]).max() <= nfr.TOL * scale
    assert np.array_equal(got["smooth_var"][3].reshape(-1), np.diag(got["c_post_cov"][3]))
    for i in (0, 4, 5):
        for key in ALL_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (i, key)
    # a C that is not positive definite: status 2 from a good linearisation; nothing observed keeps its 3
    d = CharDev(case)
    gpu_ctx.oe_nform_prepare_device(**d.prepare_args())
    d.out["h"][4] = -1e12
    bad = CharDev(case)
    bad.sa_inv = -bad.sa_inv
    gpu_ctx.oe_nform_char_device(**d.char_args())
    gpu_ctx.oe_nform_gain_device(**d.gain_args())
    gpu_ctx.oe_nform_prepare_device(**bad.prepare_args())
    gpu_ctx.oe_nform_char_device(**bad.char_args())
    gpu_ctx.oe_nform_gain_device(**bad.gain_args())
    torch.cuda.synchronize()
    got, neg = d.host(), bad.host()
    assert got["c_status"].tolist() == [1, 0, 2, 3, 2, 1]
    for key in FLOAT_KEYS:
        assert np.isnan(got[key][4]).all(), key
        assert np.array_equal(got[key][5], clean[key][5]), key
    assert neg["c_status"].tolist() == [2, 0, 2, 3, 2, 2]
    assert np.isnan(neg["c_post_cov"][3]).all() and np.isnan(neg["smooth_var"][3]).all()
    for key in ("avk", "avk_diag", "noise_var", "dfs_block", "gain"):
        assert (neg[key][3] == 0.0).all(), key
        assert np.isnan(neg[key][0]).all(), key


def test_inactive_profiles_keep_their_sentinels(gpu_ctx):
    case = seeded(43, 2, 154, True, True, 4)[0]
    full = CharDev(case).characterise(gpu_ctx)
    d = CharDev(case)
    blank = d.host()
    got = d.characterise(gpu_ctx, active=_dev(np.array([1, 0, 1, 0], dtype=np.uint8)))
    for key in ALL_KEYS:
        for i in (0, 2):
            assert np.array_equal(got[key][i], full[key][i]), (key, i)
        for i in (1, 3):
            assert np.array_equal(got[key][i], blank[key][i]), (key, i)


@pytest.mark.parametrize("shape", [(8, 1, 98), (43, 2, 154), (65, 1, 300), (128, 1, 513)], ids=lambda s: "-".join(map(str, s)))
def test_windows_batches_and_optional_outputs_leave_the_bits_alone(gpu_ctx, shape):
    nlev, nblk, m = shape
    n = nlev * nblk
    case = seeded(nlev, nblk, m, True, False, 4)[0]
    full = CharDev(case).characterise(gpu_ctx)
    # a row window of A is the slice of the full A; nothing else moves
    for rows in ((0, 1), (n - 1, 1), (n // 3, n - n // 3), (max(n - 66, 0), min(n, 5))):
        got = CharDev(case, rows=rows).characterise(gpu_ctx)
        assert np.array_equal(got["avk"], full["avk"][:, rows[0]:rows[0] + rows[1]]), rows
        for key in ALL_KEYS:
            if key != "avk":
                assert np.array_equal(got[key], full[key]), (rows, key)
    # whichever optional outputs are asked for
    for outputs in (("avk_diag",), ("dfs_block",), ("noise_var",), ("smooth_var", "c_post_cov"), ("avk", "dfs_block")):
        d = CharDev(case)
        got = d.characterise(gpu_ctx, outputs=outputs)
        for key in OPTIONAL + ("gain",):
            if key in outputs or (key == "gain" and "c_post_cov" in outputs):
                assert np.array_equal(got[key], full[key]), (outputs, key)
            else:
                assert (got[key] == -7.0).all(), (outputs, key)
        assert got["c_status"].tolist() == [1, 1, 1, 1]
    # a profile alone in its batch
    for i in (0, 3):
        one = dict(case, k=[b[i:i + 1] for b in case["k"]], x=case["x"][i:i + 1], y=case["y"][i:i + 1], fx=case["fx"][i:i + 1],
                   se=case["se"][i:i + 1])
        got = CharDev(one).characterise(gpu_ctx)
        for key in ALL_KEYS:
            assert np.array_equal(got[key][0], full[key][i]), (i, key)


def test_a_repeat_call_is_captured_and_replays_to_the_same_bits(gpu_ctx):
    """After one warm-up call (which raises the char kernel's LDS limit at n = 128) the three calls are launches alone: one
    linear chain on the capturing stream."""
    case = seeded(128, 1, 513, True, False, 4)[0]
    d = CharDev(case)
    first = d.characterise(gpu_ctx)
    d.reset()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            gpu_ctx.oe_nform_prepare_device(**d.prepare_args())
            gpu_ctx.oe_nform_char_device(**d.char_args())
            gpu_ctx.oe_nform_gain_device(**d.gain_args())
    torch.cuda.synchronize()
    assert (d.out["gain"] == -7.0).all() and (d.out["c_status"] == 9).all()      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    got = d.host()
    for key in ALL_KEYS:
        assert np.array_equal(got[key], first[key]), key


def test_argument_refusals_and_an_empty_batch(gpu_ctx):
    case = nfr.make_case(3, 3, 14, nprof=2)
    d = CharDev(case)
    rec = _native.MwrtOeNformChar
    gpu_ctx.oe_nform_prepare_device(**d.prepare_args())

    def code(entry, base, **change):
        with pytest.raises(MwrtError) as ei:
            getattr(gpu_ctx, entry)(**dict(base, **change))
        return ei.value.code, str(ei.value)

    for entry, base, required in (("oe_nform_char_device", d.char_args(), "d_h"), ("oe_nform_gain_device", d.gain_args(), "d_keep")):
        getattr(gpu_ctx, entry)(**base)                                  # the unchanged call is accepted
        assert code(entry, base, **{required: None})[0] == -1 and code(entry, base, reserved=1)[0] == -1
        assert code(entry, base, nlev=0)[0] == -1 and code(entry, base, m=0)[0] == -1 and code(entry, base, nprof=-1)[0] == -1
        assert code(entry, base, struct_size=rec.d_k.offset - 1)[0] == -1
        c, text = code(entry, base, nlev=43)                             # n = 129
        assert c == -5 and str(_native.OE_NFORM_MAX_N) in text
        getattr(gpu_ctx, entry)(**dict(base, nprof=0))                   # nothing to do is not an error
    base = d.char_args()
    assert code("oe_nform_char_device", base, row_begin=5, row_count=5)[0] == -1
    assert code("oe_nform_char_device", base, row_begin=1)[0] == -1
    assert code("oe_nform_char_device", d.char_args(outputs=()))[0] == -1
    assert code("oe_nform_char_device", base, d_avk=base["d_h"])[0] == -1
    assert code("oe_nform_gain_device", d.gain_args(), d_gain=d.gain_args()["d_post_cov"])[0] == -1
    torch.cuda.synchronize()
