"""tests/oe_exact_reference.py without a GPU: the exact reference is exact (50 and 80 digits round to the same float64, its
solve leaves no residual, it meets the NumPy references where they are good), the ladder is the ladder its docstring
promises, the pooled constants of the bars are finite and are the ones profiles/oe_conditioning_errors.json records, and
the change of units of tests/test_oe_scaling.py is the same problem to the float64 references."""
import decimal
import json
import os

import numpy as np
import pytest

import nform_reference as nfr
import oe_char_reference as ocr
import oe_exact_reference as ex
import oe_reference as oer
import whiten_reference as whr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "oe_conditioning_errors.json")
_IN = ex._IN


def _same(a, b, label):
    for key, v in a.items():
        if key in ("exact", "se_kept"):
            continue
        pairs = zip(v, b[key]) if isinstance(v, list) else [(v, b[key])]
        for x, y in pairs:
            assert np.array_equal(x, y, equal_nan=True), (label, key)


def test_fifty_and_eighty_digits_round_to_the_same_doubles():
    """Every output of a top rung of each family; the gain outputs with the m-form."""
    shape, se_full, rungs = ex.MFORM_LADDER[1]
    case = ex.mform_case(shape, se_full, rungs[-1])
    ins = {q: case[q] for q in _IN}
    _same(ex.mform_exact(**ins, gain=True), ex.mform_exact(**ins, gain=True, digits=80), "m-form")
    g = np.full(ex.NPROF, 0.5)
    _same(ex.mform_exact(**ins, gamma=g), ex.mform_exact(**ins, gamma=g, digits=80), "m-form damped")
    shape, rungs = ex.NFORM_LADDER[1]
    case = ex.nform_case(shape, rungs[-1])
    ins = {q: case[q] for q in ex.nfd_keys() + ("sa_inv",)}
    _same(ex.nform_exact(**ins), ex.nform_exact(**ins, digits=80), "n-form")
    shape, rungs = ex.WHITEN_LADDER[1]
    case = ex.whiten_case(shape, rungs[-1])
    args = (case["k"], case["se_p"], case["y"], case["fx"])
    _same(ex.whiten_exact(*args), ex.whiten_exact(*args, digits=80), "whitening")


def test_the_exact_solve_leaves_no_residual():
    """G u = d: max |G u - d| below 1e-40 at the bottom rung with 50 digits and at the top rung with 80.  At the top rung
    (cond 2e10, |G| |u| of order 1e11) no u of 50 digits can do that -- rounding u alone moves G u by 1e-50 |G| |u|; measured
    8e-40 -- so there the 50-digit residual is held to 1e-40 in its own unit, max_i (|G| |u|)_i (measured 1e-50), and the
    absolute bound to the 80-digit run that test_fifty_and_eighty_digits... shows to round to the same doubles."""
    bound = decimal.Decimal("1e-40")
    for shape, se_full, rungs in ex.MFORM_LADDER[:2]:
        for k, digits, relative in ((rungs[0], ex.DIGITS, False), (rungs[-1], 80, False), (rungs[-1], ex.DIGITS, True)):
            case = ex.mform_case(shape, se_full, k)
            out = ex.mform_exact(**{q: case[q] for q in _IN}, keep_exact=True, digits=digits)
            assert (out["cond"] >= 1e9).all() or k == rungs[0]
            with decimal.localcontext() as c:
                c.prec = 120                                                 # the residual itself adds nothing
                for e in out["exact"]:
                    G = np.tril(e["G"]) + np.tril(e["G"], -1).T            # the triangle the factorisation read
                    res = max(abs(v) for v in (G @ e["u"] - e["d"]))
                    unit = max(abs(G) @ abs(e["u"])) if relative else 1
                    print(shape, "k", k, "digits", digits, "largest |G u - d|", "%.3e" % res, "in its unit %.3e" % (res / unit))
                    assert res / unit < bound


def test_it_meets_the_numpy_references_at_the_bottom_rung():
    for shape, se_full, rungs in ex.MFORM_LADDER:
        e = ex.mform_entry((shape, se_full, rungs[0], None))
        assert (e["cond"] <= oer.COND_MAX).all() and e["numpy"]["status"].tolist() == [1] * ex.NPROF
        assert all(v <= oer.TOL for per in e["err"] for v in per.values()), (shape, e["err"])
    for shape, rungs in ex.NFORM_LADDER:
        e = ex.nform_entry((shape, rungs[0], None))
        assert (e["cond"] <= nfr.COND_MAX).all() and all(v <= nfr.TOL for per in e["err"] for v in per.values()), (shape, e["err"])
        lin = nfr.prepare_reference(**{q: e["case"][q] for q in ex.nfd_keys()})
        perr = nfr.prepare_errors(dict(h=np.stack([nfr.tri_pack(h) for h in lin["h"]]), g=lin["g"], rwr=lin["rwr"]), e["exact"])
        assert all(v <= 64 * shape[2] * ex.EPS for v in perr.values()), (shape, perr)
    for shape, rungs in ex.WHITEN_LADDER:
        e = ex.whiten_entry((shape, rungs[0]))
        assert (e["cond"] <= whr.SE_COND_MAX).all() and all(v <= whr.BAR for per in e["err"] for v in per.values()), (shape, e["err"])


@pytest.mark.parametrize("family", list(ex.FAMILIES))
def test_the_ladder_is_what_it_promises(family):
    """Bottom rung cond <= 1e4, top rung in [1e9, 1e11], no gap between neighbours wider than 1e3, NumPy's Cholesky succeeds on
    every rung (the float64 reference answers status 1 with finite numbers), no case skipped -- per profile."""
    cases, entry = ex.FAMILIES[family]
    ladders = {}
    for key in cases():
        e = entry(key)
        assert e["numpy"]["status"].tolist() == [1] * ex.NPROF and e["exact"]["status"].tolist() == [1] * ex.NPROF, key
        assert np.isfinite(e["cond"]).all() and all(np.isfinite(v) for per in e["err"] for v in per.values()), key
        if key[-1] is None or family == "whiten":                              # the damped rung is no rung of a ladder
            ladders.setdefault(key[:-1] if family == "whiten" else key[:-2], []).append(e["cond"])
    assert len(ladders) == len({"mform": ex.MFORM_LADDER, "nform": ex.NFORM_LADDER, "whiten": ex.WHITEN_LADDER}[family])
    for ladder, conds in ladders.items():
        conds = np.array(conds)                                                # [rung][profile]
        print(family, ladder, ["%.1e" % v for v in conds.max(axis=1)])
        assert (conds[0] <= ex.COND_BOTTOM).all(), ladder
        assert (conds[-1] >= ex.COND_TOP[0]).all() and (conds[-1] <= ex.COND_TOP[1]).all(), (ladder, conds[-1])
        assert (conds[1:] > conds[:-1]).all() and (conds[1:] / conds[:-1] <= ex.GAP_MAX).all(), (ladder, conds)
    if family == "mform":
        assert sorted(-(-shape[2] // 32) for shape, _, _ in ex.MFORM_LADDER) == [1, 2, 3, 4, 5]
        assert {se_full for _, se_full, _ in ex.MFORM_LADDER} == {False, True}
    damped = [key for key in cases() if family != "whiten" and key[-1] is not None]
    assert family == "whiten" or (len(damped) == 1 and damped[0][-1] > 0 and (entry(damped[0])["cond"] >= 1e8).all())


@pytest.mark.parametrize("family", list(ex.FAMILIES))
def test_the_pooled_constants_are_finite_and_the_recorded_ones(family):
    c = ex.pooled(family)
    print(family, "pooled c_out:", {k: "%.3g" % v for k, v in c.items()})
    assert c and all(np.isfinite(v) and v > 0 for v in c.values())
    with open(RECORD) as fh:
        rec = json.load(fh)["families"][family]["pooled_c"]
    assert set(rec) == set(c)
    for out, v in c.items():                                                   # to two digits
        assert abs(v - rec[out]) <= 0.01 * rec[out], (family, out, v, rec[out])


# ---- the change of units on the float64 references ----
def _back(out, D, E):
    return ex.rescale_outputs(out, D, E, inverse=True)


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_units_do_not_matter_to_the_m_form_references(se_full):
    nlev, nblk, m = 65, 2, 98
    case = oer.make_case(nlev, nblk, m, nprof=2, se_full=se_full)
    D, E = ex.unit_exponents(nblk, nlev, m)
    other = ex.rescale_case(case, D, E, se_full)
    for a, b in zip([case["x"], case["sa"], case["k"][1], case["y"]], [other["x"], other["sa"], other["k"][1], other["y"]]):
        assert (np.frexp(a)[0] == np.frexp(b)[0]).all()                        # the mantissas are untouched
    assert np.log2(D).min() >= -40 and np.log2(D).max() <= 40 and len(np.unique(D)) > 8 and len(np.unique(E)) > 8
    ref = oer.oe_step_reference(**{q: case[q] for q in _IN})
    got = _back(oer.oe_step_reference(**{q: other[q] for q in _IN}), D, E)
    assert ref["cond"].max() <= oer.COND_MAX and got["status"].tolist() == [1, 1] and got["nobs"].tolist() == [m, m]
    err = oer.block_errors(got, ref, case)
    print("step", err)
    assert all(v <= oer.TOL for v in err.values())
    ref = ocr.oe_char_reference(**{q: case[q] for q in _IN}, products=False)
    got = _back(ocr.oe_char_reference(**{q: other[q] for q in _IN}, products=False), D, E)
    err = ocr.char_errors(got, ref, case)
    print("gain", err)
    assert set(ex.GAIN_OUT) <= set(err) and all(v <= oer.TOL for v in err.values())


@pytest.mark.parametrize("se_pp", [False, True], ids=["shared", "perprofile"])
def test_units_do_not_matter_to_the_n_form_reference(se_pp):
    nlev, nblk, m = 43, 2, 60
    case = nfr.make_case(nlev, nblk, m, nprof=2, se_per_profile=se_pp)
    case["sa_inv"] = nfr.sym_inv(case["sa"])
    D, E = ex.unit_exponents(nblk, nlev, m)
    other = ex.rescale_case(case, D, E, False)
    keys = ex.nfd_keys() + ("sa_inv",)
    ref = nfr.solve_reference(**{q: case[q] for q in keys})
    got = _back(nfr.solve_reference(**{q: other[q] for q in keys}), D, E)
    assert ref["cond"].max() <= nfr.COND_MAX and got["status"].tolist() == [1, 1]
    np.testing.assert_allclose(got["cond"], ref["cond"], rtol=1e-6)            # the Jacobi-scaled C does not see the units
    err = nfr.solve_errors({q: got[q] for q in ex.NFORM_OUT}, ref, case)
    print("solve", err)
    assert all(v <= nfr.TOL for v in err.values())
    lin = nfr.prepare_reference(**{q: case[q] for q in ex.nfd_keys()})
    lin2 = _back(nfr.prepare_reference(**{q: other[q] for q in ex.nfd_keys()}), D, E)
    perr = nfr.prepare_errors(dict(h=np.stack([nfr.tri_pack(h) for h in lin2["h"]]), g=lin2["g"], rwr=lin2["rwr"]), lin)
    assert all(v <= 64 * m * ex.EPS for v in perr.values()), perr


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_units_do_not_matter_to_the_whitening_reference(se_full):
    shape = (65, 2, 65)
    nlev, nblk, m = shape
    case = whr.make_case(shape, se_full=se_full, nprof=2)
    D, E = ex.unit_exponents(nblk, nlev, m)
    other = ex.rescale_case(case, D, E, se_full)
    # With a full Se_p the float64 reference is no judge of this: it applies L^-1 with np.linalg.solve, an LU with partial
    # pivoting that does not know L is triangular, and rows scaled 2^-40 .. 2^40 apart send its pivots elsewhere (errors of
    # order 1 to 20 in these units).  The device and the exact reference substitute forwards; the exact one is used here.
    if se_full:
        ref = ex.whiten_exact(case["k"], case["se_p"], case["y"], case["fx"])
        got = _back(ex.whiten_exact(other["k"], other["se_p"], other["y"], other["fx"]), D, E)
    else:
        ref = whr.whiten_reference(case["k"], case["se_p"], case["y"], case["fx"])
        got = _back(whr.whiten_reference(other["k"], other["se_p"], other["y"], other["fx"]), D, E)
    assert ref["cond"].max() <= whr.SE_COND_MAX and got["status"].tolist() == [1, 1]
    err = {k: max(per[k] for per in ex.whiten_errors(got, ref)) for k in ex.WHITEN_OUT}
    print("whitening", err)
    assert all(v <= whr.BAR for v in err.values())
