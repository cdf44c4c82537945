"""mwrt_oe_select_device (include/mwrt.h) on the GPU against tests/select_reference.py, a longdouble
reference that recomputes q from S in every round.  Nobody is left out: every profile's order is replayed, every pick must
be within 1e-9 of the best the reference saw, every output within its bar (64 (n + nsel) eps of the bound vectors; the
docstring of select_reference derives them), and -- the margins being >= 1e-6, asserted on the CPU by
tests/test_select_reference.py -- the order must EQUAL the reference's greedy order.  Shapes: select_reference.SHAPES, held
against the plan as built by test_select_kernel_resources.py.  Every case has 4 profiles."""
import numpy as np
import pytest

import select_reference as sr
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from select_device import OPTIONAL, OUT_KEYS, SelDev, judge, profile  # noqa: E402

IDS = [f"{a}-{b}-{c}-{d}" for a, b, c, d in sr.SHAPES]


def same(a, b, keys=OUT_KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def copy_case(case):
    return {key: [b.copy() for b in v] if isinstance(v, list) else v.copy() for key, v in case.items()}


@pytest.mark.parametrize("nlev,nblk,m,nsel", sr.SHAPES, ids=IDS)
@pytest.mark.parametrize("se_pp", [False, True], ids=["shared", "seperprofile"])
def test_selection_against_the_reference(gpu_ctx, nlev, nblk, m, nsel, se_pp):
    case, greedy = sr.seeded(nlev, nblk, m, nsel, se_pp)
    assert [r["status"] for r in greedy] == [1] * sr.NPROF
    got = SelDev(case, nsel).select(gpu_ctx)
    worst = judge(case, got, greedy, nsel, label=(nlev, nblk, m, nsel, se_pp))
    assert max(worst.values()) <= 1.0, worst
    for i in range(sr.NPROF):
        assert np.array_equal(got["post_cov"][i], got["post_cov"][i].T)
        assert np.array_equal(got["post_var"][i].reshape(-1), np.diag(got["post_cov"][i]))
        chosen = got["rank"][i] >= 0
        assert np.array_equal(got["q"][i][got["order"][i]], got["q_pick"][i]) and chosen.sum() == got["count"][i]


def test_identical_rows_tie_to_the_lowest_index(gpu_ctx):
    """Rows 3 and 11 bit-identical with equal variances: 3 goes first, and 11's q afterwards is q / (1 + q) of its value
    before (the closed form of one assimilation of the same row), within the bar.  Then three identical rows."""
    nlev, nblk, m, nsel = 12, 2, 40, 6
    n = nblk * nlev
    base = sr.make_case(nlev, nblk, m)
    for twins in ((3, 11), (3, 11, 29)):
        case = copy_case(base)
        for b in case["k"]:
            b[:, 3] *= 40.0                                             # the strongest row by far: picked first
            for j in twins[1:]:
                b[:, j] = b[:, 3]
        got = SelDev(case, nsel).select(gpu_ctx)
        greedy = sr.select_batch(case, nsel)
        for i in range(sr.NPROF):
            g = profile(got, i)
            assert g["status"] == 1 and g["order"][0] == 3, g["order"]
            # after the pick of 3 the twins hold q0 / (1 + q0) and still tie: the next of them is again the lowest index,
            # whenever a twin is picked at all
            later = [j for j in g["order"][1:] if j in twins]
            assert later == sorted(later), g["order"]
            rep = sr.replay(case, i, g["order"], greedy[i])
            err = sr.select_errors(g, rep, n, case["s0"])
            assert max(err.values()) <= 1.0, err
        # one round alone: the twin's q after the first pick against the closed form
        one = SelDev(case, 1).select(gpu_ctx)
        f = sr.bar_factor(n, 1)
        for i in range(sr.NPROF):
            o = profile(one, i)
            q0 = o["q_pick"][0]
            assert o["order"][0] == 3
            for j in twins[1:]:
                assert o["q"][j] != 0.0 and abs(o["q"][j] - q0 / (1.0 + q0)) <= f * greedy[i]["b"][j], (i, j, o["q"][j], q0)
                assert o["q"][j] == o["q"][twins[1]]                    # bit for bit among the twins


def test_a_zero_row_is_never_picked(gpu_ctx):
    nlev, nblk, m = 8, 1, 6
    case = copy_case(sr.make_case(nlev, nblk, m))
    case["k"][0][:, 2] = 0.0
    got = SelDev(case, m).select(gpu_ctx)
    greedy = sr.select_batch(case, m)
    worst = judge(case, got, greedy, m, label="zero row")
    assert max(worst.values()) <= 1.0
    assert (got["count"] == m - 1).all() and (got["order"][:, -1] == -1).all() and (got["rank"][:, 2] == -1).all()
    assert (got["q_pick"][:, -1] == 0.0).all() and (got["dfs_gain"][:, -1] == 0.0).all() and (got["q"][:, 2] == 0.0).all()
    assert got["status"].tolist() == [1] * sr.NPROF


def test_a_nan_removes_its_row_alone(gpu_ctx):
    """A NaN in a row of K, and one in a variance, in profile 1: the other outputs are bit-identical to a run with those rows
    switched off in d_keep, and the neighbours never see it."""
    nlev, nblk, m, nsel = 33, 1, 141, 20
    base, _ = sr.seeded(nlev, nblk, m, nsel, True)
    clean = SelDev(base, nsel).select(gpu_ctx)
    case = copy_case(base)
    case["k"][0][1, 17, 5] = np.nan
    case["se"][1, 140] = np.nan
    keep = np.ones((sr.NPROF, m), dtype=np.uint8)
    keep[1, [17, 140]] = 0
    got = SelDev(case, nsel).select(gpu_ctx)
    masked = SelDev(base, nsel, keep=keep).select(gpu_ctx)
    same(got, masked)
    for i in (0, 2, 3):
        same(profile(got, i), profile(clean, i))
    assert (got["q"][1, [17, 140]] == 0.0).all() and (got["rank"][1, [17, 140]] == -1).all()
    worst = judge(case, got, sr.select_batch(case, nsel), nsel, label="nan rows")
    assert max(worst.values()) <= 1.0, worst


def test_keep_and_candidate_switch_rows_off(gpu_ctx):
    nlev, nblk, m, nsel = 12, 2, 224, 24
    case, greedy = sr.seeded(nlev, nblk, m, nsel)
    keep = np.ones((sr.NPROF, m), dtype=np.uint8)
    cand = np.ones(m, dtype=np.uint8)
    for i in range(sr.NPROF):
        keep[i, greedy[i]["order"][:3]] = 0                             # the three best of every profile
    cand[::2] = 0
    got = SelDev(case, nsel, keep=keep, candidate=cand).select(gpu_ctx)
    ref = sr.select_batch(case, nsel, keep=keep, candidate=cand)
    worst = judge(case, got, ref, nsel, keep=keep, candidate=cand, label="masks")
    assert max(worst.values()) <= 1.0, worst
    off = (keep == 0) | (cand == 0)[None, :]
    assert (got["rank"][off] == -1).all() and (got["q"][off] == 0.0).all()


def test_shared_and_per_profile_inputs_agree_bit_for_bit(gpu_ctx):
    nlev, nblk, m, nsel = 16, 2, 50, 12
    case = sr.make_case(nlev, nblk, m)
    wide = copy_case(case)
    wide["s0"] = np.broadcast_to(case["s0"], (sr.NPROF,) + case["s0"].shape).copy()
    wide["se"] = np.broadcast_to(case["se"], (sr.NPROF, m)).copy()
    same(SelDev(case, nsel).select(gpu_ctx), SelDev(wide, nsel).select(gpu_ctx))


def test_status_values_beside_a_good_profile(gpu_ctx):
    nlev, nblk, m, nsel, nprof = 16, 2, 20, 8, 6
    base = sr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=True)
    base["s0"] = np.broadcast_to(base["s0"], (nprof,) + base["s0"].shape).copy()
    clean = SelDev(base, nsel).select(gpu_ctx)
    case = copy_case(base)
    case["s0"][1, 3, 2] = np.nan                                        # status 0
    case["se"][2, 7] = -0.25                                            # status 2: a candidate's variance
    for b in case["k"]:
        b[3] = np.nan                                                   # status 3: no candidate
    case["s0"][4] = np.diag(np.diag(case["s0"][4]))
    for b in case["k"]:
        b[4, 0] *= 1e200                                                # status 2: row 0 is picked and its d is not finite
    ref = sr.select_batch(case, nsel)
    assert [r["status"] for r in ref] == [1, 0, 2, 3, 2, 1]
    got = SelDev(case, nsel).select(gpu_ctx)
    worst = judge(case, got, ref, nsel, label="statuses")
    assert max(worst.values()) <= 1.0, worst
    g = profile(got, 3)
    assert g["count"] == 0 and (g["order"] == -1).all() and (g["rank"] == -1).all() and (g["q"] == 0.0).all()
    assert np.array_equal(g["post_cov"], case["s0"][3]) and np.array_equal(g["post_var"].reshape(-1), np.diag(case["s0"][3]))
    for i in (0, 5):
        same(profile(got, i), profile(clean, i))
    # a NaN in Sa^-1 fails every profile, but only when Sa^-1 is read
    case = copy_case(base)
    case["sa_inv"] = case["sa_inv"].copy()
    case["sa_inv"][0, 1] = np.nan
    d = SelDev(case, nsel)
    assert d.select(gpu_ctx)["status"].tolist() == [0] * nprof
    d.reset()
    without = d.select(gpu_ctx, outputs=("post_cov", "post_var"))
    same(without, clean, keys=("order", "q_pick", "rank", "q", "count", "status", "post_cov", "post_var"))


def test_inactive_profiles_keep_their_sentinels(gpu_ctx):
    nlev, nblk, m, nsel = 43, 2, 60, 10
    case = sr.make_case(nlev, nblk, m)
    full = SelDev(case, nsel).select(gpu_ctx)
    d = SelDev(case, nsel, active=[1, 0, 1, 0])
    blank = d.host()
    got = d.select(gpu_ctx)
    for i in (1, 3):
        same(profile(got, i), profile(blank, i))
    for i in (0, 2):
        same(profile(got, i), profile(full, i))


def test_outputs_do_not_depend_on_the_batch_or_the_optional_outputs(gpu_ctx):
    nlev, nblk, m, nsel = 65, 1, 90, 16
    case = sr.make_case(nlev, nblk, m, nprof=5, se_per_profile=True)
    full = SelDev(case, nsel).select(gpu_ctx)
    required = ("order", "q_pick", "rank", "q", "count", "status")
    for outputs in ((), ("dfs_gain",), ("post_cov",), ("post_var",)):
        d = SelDev(case, nsel)
        got = d.select(gpu_ctx, outputs=outputs)
        same(got, full, keys=required + outputs)
        for key in OPTIONAL:
            if key not in outputs:
                assert np.isnan(got[key]).all(), key                    # the sentinel: never written
    # profile 3 alone (nprof 1), and at another index of a reversed batch
    one = {key: [b[3:4].copy() for b in v] if isinstance(v, list) else (v[3:4].copy() if key == "se" else v)
           for key, v in case.items()}
    same(profile(SelDev(one, nsel).select(gpu_ctx), 0), profile(full, 3))
    rev = {key: [b[::-1].copy() for b in v] if isinstance(v, list) else (v[::-1].copy() if key == "se" else v)
           for key, v in case.items()}
    back = SelDev(rev, nsel).select(gpu_ctx)
    for i in range(5):
        same(profile(back, 4 - i), profile(full, i))


def test_the_entry_replays_from_a_hip_graph(gpu_ctx):
    """One capture after a warm-up call at n = 125, above the 64-KiB raise of the LDS limit, replayed once: bit for bit."""
    nlev, nblk, m, nsel = 125, 1, 31, 12
    case, _ = sr.seeded(nlev, nblk, m, nsel)
    d = SelDev(case, nsel)
    eager = d.select(gpu_ctx)                                           # the warm-up: the limit is raised here
    d.reset()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            gpu_ctx.oe_select_device(**d.args())
    torch.cuda.synchronize()
    assert np.isnan(d.host()["q_pick"]).all()                           # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    same(d.host(), eager)


def test_refusals_write_nothing(gpu_ctx):
    case = sr.make_case(8, 1, 20)
    d = SelDev(case, 5)
    blank = d.host()
    for change, needle in ((dict(nsel=0), "nsel"), (dict(nsel=21), "nsel"), (dict(d_s0=None), "null buffer"),
                           (dict(d_sa_inv=None), "d_dfs_gain"), (dict(d_q=d.se.data_ptr()), "equals an input"),
                           (dict(reserved=1), "reserved")):
        with pytest.raises(MwrtError, match=needle):
            gpu_ctx.oe_select_device(**dict(d.args(), **change))
    big = SelDev(sr.make_case(65, 2, 4), 2)
    with pytest.raises(MwrtError, match="MWRT_OE_NFORM_MAX_N \\(128"):
        gpu_ctx.oe_select_device(**big.args())
    gpu_ctx.oe_select_device(**dict(d.args(), nprof=0))
    torch.cuda.synchronize()
    same(d.host(), blank)
