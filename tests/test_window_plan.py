"""The window plan of the fine-grid absorption kernel, read in full (tests/plan_dump.cpp `windows`, the planning unit linked
as is and run under ASan + UBSan) and held to tests/window_reference.py over the geometry table of tests/window_cases.py,
for R98, R17 and R24: the structure of the plan and every far-set / LineMasks bit against the restated rules, the three
kinds of Lagrange weights against what they must reproduce, and the accuracy the plan alone leaves (``plan_truncation``)
against half of the 1e-9 absorption bar.  No GPU.

Measured, worst over the table (profiles/window_geometry_errors.json, "reference"): dry 2.7e-10 (118-far-above, R24: the
118.75-GHz line 4.01 GHz beyond a 5-GHz window, 2.6 half-spans from its middle), wet 1.2e-13, half-sampled speed-dependent
shape 1.5e-12 (sdint-at-5-spans)."""
import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
from plan_dump_tool import plan_dump, request          # noqa: F401 (plan_dump: the fixture, sanitised build)
import window_cases as wc
import window_reference as wr

LD = np.longdouble
TRUNCATION_BAR = 5e-10        # half of the 1e-9 absorption bar against the oracle; the other half is the device's rounding


@pytest.fixture(scope="module")
def plans(plan_dump, tmp_path_factory):
    """{(case name, model name): plan} for the whole table, from one sanitised run per model"""
    out = {}
    for name in wc.CPU_MODELS:
        path = tmp_path_factory.mktemp("desc") / (name + ".desc")
        path.write_bytes(bytes(sp.get_model(name).to_c()))
        asked = [request("tables", path)] + [request("windows", *c.frq) for c in wc.CASES] + \
                [request("eligible", *c.frq) for c in wc.CASES]
        got = plan_dump(asked)
        n = len(wc.CASES)
        for c, dump, el in zip(wc.CASES, got[1:1 + n], got[1 + n:]):
            out[c.name, name] = dict(wr.plan_arrays(dump, c.frq), eligible=el["eligible"])
    return out


def every(plans):
    return [(wc.BY_NAME[c], sp.get_model(mn), plan) for (c, mn), plan in plans.items()]


def test_every_case_reaches_its_branch(plans):
    for case, m, plan in every(plans):
        assert plan["eligible"] == case.eligible == wr.eligible(case.frq), case.name
        assert plan["packed"] and plan["nf"] == len(case.frq)
        wc.reaches(case, m, plan)
    # the near case differs from the far case in the 118-GHz bit alone
    for mn in wc.CPU_MODELS:
        a, b = plans["118-far-below", mn]["windows"][0], plans["118-near-below", mn]["windows"][0]
        assert bin(a["o2_far"] ^ b["o2_far"]).count("1") == 1 and (a["h2o_far_both"], a["h2o_far_res"]) == (b["h2o_far_both"], b["h2o_far_res"])


def test_windows_cover_the_chunks_and_merge_by_the_rule(plans):
    for case, m, plan in every(plans):
        nf = len(case.frq)
        nchunks = -(-nf // 16)
        wins = plan["windows"]
        want = wr.spans_of(m, [float(x) for x in case.frq])
        # dispatch order: a permutation of the windows the rule gives, in whatever order
        assert sorted((w["first_chunk"], w["nchunks"]) for w in wins) == want, (case.name, m.name)
        covered = sorted(ch for w in wins for ch in range(w["first_chunk"], w["first_chunk"] + w["nchunks"]))
        assert covered == list(range(nchunks)), (case.name, m.name)
        assert all(1 <= w["nchunks"] <= 16 for w in wins)
        base = wr.base_spans(nf)
        for a, b in zip(base, base[1:]):                         # merged exactly where the rule allows (left to right)
            merged = any(w["first_chunk"] == a[0] and w["nchunks"] == a[1] + b[1] for w in wins)
            inside = any(w["first_chunk"] < a[0] < w["first_chunk"] + w["nchunks"] for w in wins)    # a is the tail of a merge
            assert merged == (wr.may_merge(m, case.frq, a, b) and not inside), (case.name, m.name, a, b)
        for w in wins:
            b, e = wr.bounds((w["first_chunk"], w["nchunks"]), nf)
            assert w["flo"] == case.frq[b] and w["fhi"] == case.frq[e], (case.name, m.name)


def test_far_sets_and_masks_equal_the_restatement(plans):
    for case, m, plan in every(plans):
        for w in plan["windows"]:
            assert (w["o2_far"], w["h2o_far_both"], w["h2o_far_res"]) == wr.far_sets(m, w["flo"], w["fhi"]), (case.name, m.name)
        want = wr.chunk_masks(m, case.frq)
        assert len(plan["masks"]) == len(want)
        for ch, (g, r) in enumerate(zip(plan["masks"], want)):
            assert g == r, (case.name, m.name, ch, {k: (g[k], r[k]) for k in r if g[k] != r[k]})


def normalised(f, lo, hi):
    lo, hi = LD(lo), LD(hi)
    return (np.asarray(f, dtype=LD) - 0.5 * (lo + hi)) / (0.5 * (hi - lo))


def reproduction_error(nodes, targets, weights, degree, lo, hi):
    """largest |sum_m w[m][j] T_k(x_m) - T_k(x_j)| over Chebyshev polynomials T_0 .. T_degree of the coordinate that maps
    [lo, hi] to [-1, 1]; weights [node][target]"""
    xn, xt = normalised(nodes, lo, hi), normalised(targets, lo, hi)
    cheb = np.polynomial.chebyshev.chebvander
    vn, vt = cheb(xn, degree).astype(LD), cheb(xt, degree).astype(LD)                 # (chebvander keeps the extended type)
    return float(np.max(np.abs(weights.astype(LD).T @ vn - vt)))


def test_weights_reproduce_polynomials(plans):
    """every Lagrange block: finite, each target's weights sum to 1, polynomials of degree <= 15 / 7 / 8 in the window's
    (chunk's) normalised coordinate reproduced, [chunk][node][target], pad targets = last frequency, node hits = unit columns"""
    for case, m, plan in every(plans):
        frq, nf = plan["frq"], len(plan["frq"])
        key = (case.name, m.name)
        assert np.isfinite(plan["lag_sd"]).all(), key
        for w in plan["windows"]:
            assert w["lag_rest_zero"], key
            idx = wr.window_targets(plan, w)
            padded = np.minimum(np.arange(w["first_chunk"] * 16, (w["first_chunk"] + w["nchunks"]) * 16), nf - 1)
            for nodes, block, n in ((w["fnode"], w["lag"], 16), (w["fnode_h"], w["lag_h"], 8)):
                nodes = np.array(nodes)
                assert np.isfinite(block).all() and np.isfinite(nodes).all(), key
                ref = wr.chebyshev_nodes(w["flo"], w["fhi"], n)
                assert np.all(np.abs(nodes - ref) <= np.spacing(w["fhi"])), key         # Chebyshev nodes, to the last bit but one
                assert np.all(np.diff(nodes) < 0) and w["flo"] <= nodes[-1] and nodes[0] <= w["fhi"], key
                flat = np.transpose(block, (1, 0, 2)).reshape(n, -1)                    # [node][target of the window]
                assert np.abs(flat.astype(LD).sum(axis=0) - 1).max() <= 1e-13, key
                assert reproduction_error(nodes, frq[padded], flat, n - 1, w["flo"], w["fhi"]) <= 1e-11, key
                assert np.array_equal(flat[:, len(idx):], np.repeat(flat[:, len(idx) - 1:len(idx)], flat.shape[1] - len(idx), axis=1)), key
                for j in np.nonzero(np.isin(frq[padded], nodes))[0]:
                    assert np.array_equal(flat[:, j], (nodes == frq[padded][j]).astype(float)), key
        for ch in range(len(plan["masks"])):
            f = frq[ch * 16:(ch + 1) * 16]
            wsd = plan["lag_sd"][ch]                                                    # [target][node]
            if not wr.sd_half_ok(f):                                                    # never half-sampled: no weights
                assert not wsd.any() and not plan["masks"][ch]["h2o_sdint"], key
                continue
            nodes, tg = f[list(wr.SD_NODE_SLOTS)], f[list(wr.SD_TARGET_SLOTS)]
            assert np.abs(wsd.astype(LD).sum(axis=1) - 1).max() <= 1e-13, key
            assert reproduction_error(nodes, tg, wsd.T, 8, f[0], f[-1]) <= 1e-11, (key, ch)


def test_a_target_on_a_node_gets_a_unit_column(plan_dump, tmp_path):
    """a list that contains the window's own Chebyshev nodes: those targets read their node alone"""
    m = sp.get_model("R24")
    path = tmp_path / "R24.desc"
    path.write_bytes(bytes(m.to_c()))
    base = np.linspace(30.0, 35.0, 128)
    nodes = np.asarray(wr.chebyshev_nodes(30.0, 35.0, 16), dtype=np.float64)
    first = plan_dump([request("tables", path), request("windows", *base)])[1]["windows"][0]
    frq = np.sort(np.concatenate([base[:1], first["fnode"][2:7], base[1:-6], base[-1:]]))       # five of the dumped nodes as targets
    assert len(frq) == 128 and np.all(np.diff(frq) > 0) and np.allclose(first["fnode"], nodes, rtol=0, atol=1e-14)
    plan = wr.plan_arrays(plan_dump([request("tables", path), request("windows", *frq)])[1], frq)
    w = plan["windows"][0]
    flat = np.transpose(w["lag"], (1, 0, 2)).reshape(16, -1)
    hits = np.nonzero(np.isin(frq, w["fnode"]))[0]
    assert len(hits) == 5
    for j in hits:
        assert np.array_equal(flat[:, j], (np.array(w["fnode"]) == frq[j]).astype(float))


SAMPLE_LEVELS = (0, 1, 60, 120, 176, 177, 178, 179)       # bottom two, two middle, top four of 180


@pytest.fixture(scope="module")
def truncation(plans):
    """plan_truncation of every (case, model) over the sample levels of three profiles -> {(case, model): dict}"""
    column = sample_levels()
    return {(cn, mn): wr.plan_truncation(plan, sp.get_model(mn), column) for (cn, mn), plan in plans.items()}


def sample_levels():
    """the sample levels of the three profiles as one 24-level column (the levels are independent of each other)"""
    P = pr.synthetic_profiles(3, 5)
    return {k: np.concatenate([P[k][i][list(SAMPLE_LEVELS)] for i in range(3)]) for k in ("p", "t", "rh")}


def test_plan_truncation_stays_under_half_the_absorption_bar(truncation):
    print("\nplan truncation, relative to the total dry / wet absorption (bar %.0e):" % TRUNCATION_BAR)
    for (cn, mn), r in sorted(truncation.items()):
        print("  %-24s %-4s dry %.2e  wet %.2e  sd %.2e" % (cn, mn, r["dry"], r["wet"], r["sd"]))
    over = {k: r for k, r in truncation.items() if max(r.values()) > TRUNCATION_BAR}
    assert not over, over
    # the cases are in the table because the plan is strained there: the 118-GHz line at 2.6 half-spans leaves an error
    # far above rounding, the quiet stretch of the band does not
    assert truncation["span-limit", "R24"]["dry"] > 1e-10 > truncation["merge-partial", "R24"]["dry"]


@pytest.mark.parametrize("species, case", [("o2", "span-limit"), ("h2o", "118-far-below")])
def test_truncation_figure_holds_in_mpmath(plans, species, case):
    """one geometry per species with every step at 30 digits: the extended-precision figure is the figure"""
    m = sp.get_model("R24")
    plan = plans[case, "R24"]
    P = pr.synthetic_profiles(3, 5)
    w = plan["windows"][0]
    idx = wr.window_targets(plan, w)[::9]
    exact, ld = wr.confirm_with_mpmath(m, {k: P[k][1] for k in ("p", "t", "rh")}, 179, w, idx, plan["frq"], species)
    assert exact > 1e-13 and abs(ld - exact) <= 1e-3 * exact, (exact, ld)


def test_speed_dependent_line_is_taken_back_from_the_far_set(plans):
    """The host puts the 22-GHz line in the window's far set by its half-width bound.  With ground levels at 150 K,
    saturated, ten ACTUAL half-widths (the oracle's width formula) stay short of the window at 2000 hPa -- 9.2 GHz of half
    width against the bound's 9.8 -- and reach it at 2500 hPa: there the kernel's per-level vote must take the line back.
    No level of the unmodified profiles comes near."""
    m = sp.get_model("R24")
    k = wc.line_bit(m.h2o["fl"], wc.H2O_22).bit_length() - 1
    for name, taken in (("sd-heavy-ground-2000", False), ("sd-taken-back", True)):
        w = plans[name, "R24"]["windows"][0]
        assert w["h2o_far_both"] >> k & 1
        P = wc.heavy_ground(pr.synthetic_profiles(3, 5), wc.BY_NAME[name].heavy_hpa)
        reach, centre = wr.sd_reach(m, P["p"][1], P["t"][1], P["rh"][1], k)
        dist = np.minimum(np.abs(centre - w["flo"]), np.abs(centre - w["fhi"]))
        assert (reach[:3] > dist[:3]).all() == taken and (reach[:3] > 0.9 * dist[:3]).all(), (name, reach[:3], dist[:3])
        assert (reach[3:] < 0.5 * dist[3:]).all()
        assert (10.0 * wr.sd_halfwidth_bound(m, k) < dist - 1.0).all()
        assert (reach[:3] > 10.0 * wr.sd_halfwidth_bound(m, k)).all() == taken
