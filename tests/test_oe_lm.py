"""mwrt_oe_lm_prepare_device, mwrt_oe_lm_solve_device and mwrt_oe_cost_device (include/mwrt.h) on the GPU against
tests/oe_lm_reference.py, and OneDVar.retrieve_lm on the real operator.

Tolerances (derived, not measured):
  r            y - fx is one subtraction on both sides: equal.
  K dx, G0     sums of n (and n x n) products in a fixed order: the forward error bound of nested length-n sums,
               2 n eps (|K| |dx|)_i and 2 n eps (|K| |Sa| |K|^T)_ij per entry, computed by the reference.  No mask, no floor.
  x+, chi2     Cholesky + solves are backward stable, error <~ 64 m eps cond(G_gamma) <= oe_reference.TOL with cond <= 1e4
               asserted on the reference's G_gamma per case; in the units of oe_reference.block_errors.
  J prior      2 n eps |dx|^T |Sa^-1| |dx|;  J obs  TOL max(1, J_obs) (cond(Se) <= 4 asserted).
Shapes are oe_reference.SHAPES.  What they reach is asserted by
test_oe_shape_coverage.py::test_the_shapes_reach_what_they_are_for against the code's own LDS plans and dispatch rule, and
that test is the authority: k_lm_prepare<1 .. 5> with both sides of every tile edge, m = 1 and the m limit, one to four K
blocks, both sides of the register seams of k_lm_solve's wave 0 (m = 64 | 65, 128 | 129), both sides of the first raise of
each kernel's LDS limit at n = 130 (prepare m = 69 | 70, cost with a full Se 122 | 123, solve 124 | 125), and the two shapes
whose x - xa outgrows the panel buffers of k_lm_prepare (n = 2100, 3636).  Rows are dropped at m = 98 and, on the tile and
register seams, at m = 65 (oe_reference.SEAM_DROPS)."""
import numpy as np
import pytest

import oe_lm_reference as lmr
import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LIN_KEYS = ("g0", "r", "kdx", "keep", "lin_status")
SOLVE_KEYS = ("x_new", "status", "chi2", "nobs")
COST_KEYS = ("cost", "cost_obs", "cost_prior", "cost_status")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


_inverses = []


def sym_inv(sa):
    """The symmetrised inverse of Sa, computed once per array object (a 3636 x 3636 inverse takes longer than every
    kernel of its case); nobody writes to either."""
    for held, inv in _inverses:
        if held is sa:
            return inv
    inv = np.linalg.inv(sa)
    inv = 0.5 * (inv + inv.T)
    _inverses.append((sa, inv))
    return inv


class Dev:
    """A case of oe_reference.make_case on the device with every output of the three calls pre-filled with a sentinel, so
    an entry a kernel leaves unwritten shows."""

    def __init__(self, case, gamma=0.0):
        self.k = [_dev(b) for b in case["k"]]
        self.nprof, self.m, self.nlev = self.k[0].shape
        self.nblk = len(self.k)
        self.x, self.xa, self.sa, self.se, self.y, self.fx = (_dev(case[key]) for key in ("x", "xa", "sa", "se", "y", "fx"))
        self.sa_inv = _dev(sym_inv(case["sa"]))
        self.gamma = _dev(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.nprof,)).copy())
        self.flags = dict(xa_per_profile=case["xa"].ndim == 3, se_full=case["se"].ndim == 2)
        self.reset()

    def reset(self):
        f64, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.uint8, device="cuda")
        nprof, m = self.nprof, self.m
        self.out = dict(g0=torch.full((nprof, m * (m + 1) // 2), -7.0, **f64), r=torch.full((nprof, m), -7.0, **f64),
                        kdx=torch.full((nprof, m), -7.0, **f64), keep=torch.full((nprof, m), 9, **u8),
                        lin_status=torch.full((nprof,), 9, **u8),
                        x_new=torch.full((nprof, self.nblk, self.nlev), -7.0, **f64), status=torch.full((nprof,), 9, **u8),
                        chi2=torch.full((nprof,), -7.0, **f64), nobs=torch.full((nprof,), -7, dtype=torch.int32, device="cuda"),
                        cost=torch.full((nprof,), -7.0, **f64), cost_obs=torch.full((nprof,), -7.0, **f64),
                        cost_prior=torch.full((nprof,), -7.0, **f64), cost_status=torch.full((nprof,), 9, **u8))

    def _lin(self):
        return {"d_" + key: self.out[key].data_ptr() for key in LIN_KEYS}

    def prepare_args(self, active=None, stream=None):
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, d_k=[b.data_ptr() for b in self.k], d_x=self.x.data_ptr(),
                    d_xa=self.xa.data_ptr(), d_sa=self.sa.data_ptr(), d_se=self.se.data_ptr(), d_y=self.y.data_ptr(),
                    d_fx=self.fx.data_ptr(), d_active=None if active is None else active.data_ptr(),
                    stream=_cur() if stream is None else stream, **self._lin(), **self.flags)

    def solve_args(self, active=None, stream=None):
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, d_k=[b.data_ptr() for b in self.k], d_x=self.x.data_ptr(),
                    d_xa=self.xa.data_ptr(), d_sa=self.sa.data_ptr(), d_se=self.se.data_ptr(), d_gamma=self.gamma.data_ptr(),
                    d_x_new=self.out["x_new"].data_ptr(), d_status=self.out["status"].data_ptr(),
                    d_chi2=self.out["chi2"].data_ptr(), d_nobs=self.out["nobs"].data_ptr(),
                    d_active=None if active is None else active.data_ptr(), stream=_cur() if stream is None else stream,
                    **self._lin(), **self.flags)

    def cost_args(self, active=None, stream=None):
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, nblk=self.nblk, d_x=self.x.data_ptr(), d_xa=self.xa.data_ptr(),
                    d_se=self.se.data_ptr(), d_y=self.y.data_ptr(), d_fx=self.fx.data_ptr(), d_keep=self.out["keep"].data_ptr(),
                    d_sa_inv=self.sa_inv.data_ptr(), d_cost=self.out["cost"].data_ptr(), d_cost_obs=self.out["cost_obs"].data_ptr(),
                    d_cost_prior=self.out["cost_prior"].data_ptr(), d_status=self.out["cost_status"].data_ptr(),
                    d_active=None if active is None else active.data_ptr(), stream=_cur() if stream is None else stream,
                    **self.flags)

    def run(self, ctx, active=None):
        """prepare, solve, cost back to back -> dict of NumPy outputs."""
        ctx.oe_lm_prepare_device(**self.prepare_args(active))
        ctx.oe_lm_solve_device(**self.solve_args(active))
        ctx.oe_cost_device(**self.cost_args(active))
        torch.cuda.synchronize()
        return self.host()

    def host(self):
        return {key: v.cpu().numpy() for key, v in self.out.items()}


def reference(case, gamma):
    keep_case = {key: case[key] for key in ("k", "x", "xa", "sa", "se", "y", "fx")}
    lin = lmr.prepare_reference(**keep_case)
    sol = lmr.solve_reference(gamma=gamma, **keep_case)
    cost = lmr.cost_reference(case["x"], case["xa"], case["se"], case["y"], case["fx"], lin["keep"], sym_inv(case["sa"]))
    return lin, sol, cost


def check_prepare(got, lin, label):
    assert got["keep"].tolist() == lin["keep"].tolist() and got["lin_status"].tolist() == lin["lin_status"].tolist(), label
    ok = lin["lin_status"] == 1
    assert np.array_equal(got["r"][ok], lin["r"][ok]), label
    e_k = np.abs(got["kdx"][ok] - lin["kdx"][ok])
    assert (e_k <= lin["kdx_bound"][ok]).all(), (label, float((e_k / np.maximum(lin["kdx_bound"][ok], 1e-300)).max()))
    worst = 0.0
    for i in np.flatnonzero(ok):
        e_g = np.abs(got["g0"][i] - lmr.tri_pack(lin["g0"][i]))
        bound = lmr.tri_pack(lin["g0_bound"][i])
        assert (e_g <= bound).all(), (label, i, float(e_g.max()))
        worst = max(worst, float((e_g[bound > 0] / bound[bound > 0]).max()))
    print(label, "G0 error / bound", worst)


def check_solve(got, sol, case, label):
    assert got["status"].tolist() == sol["status"].tolist() and got["nobs"].tolist() == sol["nobs"].tolist(), label
    ok = sol["status"] == 1
    assert ok.any() and np.nanmax(sol["cond"]) <= oer.COND_MAX, (label, sol["cond"])
    err = oer.block_errors(dict(x_new=got["x_new"], chi2=got["chi2"]), sol, case)
    print(label, "solve", err)
    assert np.isfinite(got["x_new"][ok]).all() and np.isfinite(got["chi2"][ok]).all(), label
    assert err["x_new"] <= oer.TOL and err["chi2"] <= oer.TOL, (label, err)


def check_cost(got, cost, label):
    assert got["cost_status"].tolist() == cost["status"].tolist(), label
    fin = np.isfinite(cost["cost"])
    assert fin.any() and np.nanmax(cost["cond"]) <= 4.0, (label, cost["cond"])
    e_p = np.abs(got["cost_prior"][fin] - cost["prior"][fin])
    e_o = np.abs(got["cost_obs"][fin] - cost["obs"][fin])
    print(label, "cost: prior error / bound", float((e_p / cost["prior_bound"][fin]).max()), "obs error",
          float((e_o / np.maximum(1.0, cost["obs"][fin])).max()))
    assert (e_p <= cost["prior_bound"][fin]).all(), label
    assert (e_o <= oer.TOL * np.maximum(1.0, cost["obs"][fin])).all(), label
    assert np.array_equal(got["cost"][fin], got["cost_obs"][fin] + got["cost_prior"][fin]), label
    for key in ("cost", "cost_obs", "cost_prior"):
        assert np.array_equal(got[key][~fin], cost["cost"][~fin], equal_nan=True), (label, key)


_cases = {}


def seeded(nlev, nblk, m, se_full, xa_pp, nprof):
    key = (nlev, nblk, m, se_full, xa_pp, nprof)
    if key not in _cases:
        case = oer.make_case(nlev, nblk, m, nprof=nprof, se_full=se_full, xa_per_profile=xa_pp)
        gammas = [np.array(lmr.GAMMAS[:nprof])] + ([np.array(lmr.GAMMAS[-nprof:])] if nprof < len(lmr.GAMMAS) else [])
        _cases[key] = (case, gammas, [reference(case, g) for g in gammas])
    return _cases[key]


def _copy(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else [b.copy() for b in v]) for k, v in case.items()}


@pytest.mark.parametrize("nlev,nblk,m", oer.SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in oer.SHAPES])
@pytest.mark.parametrize("se_full,xa_pp", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["diag-shared", "full-shared", "diag-perprofile", "full-perprofile"])
def test_prepare_solve_and_cost_against_the_reference(gpu_ctx, nlev, nblk, m, se_full, xa_pp):
    nprof = 3 if nlev >= 180 else 4
    case, gammas, refs = seeded(nlev, nblk, m, se_full, xa_pp, nprof)
    label = (nlev, nblk, m, se_full, xa_pp)
    for gamma, (lin, sol, cost) in zip(gammas, refs):                    # gamma = (0, 0.25, 4, 1e3) across the profiles
        d = Dev(case, gamma)
        got = d.run(gpu_ctx)
        check_prepare(got, lin, label)
        check_solve(got, sol, case, label + (tuple(gamma),))
        check_cost(got, cost, label)
    # gamma = 0 is mwrt_oe_step_device on the same inputs (profile 0 of the first run)
    d = Dev(case, gammas[0])
    got = d.run(gpu_ctx)
    step = torch.full_like(d.out["x_new"], -7.0)
    status = torch.zeros(nprof, dtype=torch.uint8, device="cuda")
    gpu_ctx.oe_step_device(nprof, nlev, m, [b.data_ptr() for b in d.k], d.x.data_ptr(), d.xa.data_ptr(), d.sa.data_ptr(),
                           d.se.data_ptr(), d.y.data_ptr(), d.fx.data_ptr(), step.data_ptr(), status.data_ptr(), stream=_cur(),
                           **d.flags)
    torch.cuda.synchronize()
    step = step.cpu().numpy()
    xa = np.broadcast_to(case["xa"], step.shape)
    diff = max(float(np.abs(got["x_new"][0, b] - step[0, b]).max() / np.abs(refs[0][1]["x_new"][0, b] - xa[0, b]).max())
               for b in range(nblk))
    print(label, "gamma = 0 against mwrt_oe_step_device:", diff)
    assert diff <= oer.TOL, (label, diff)


@pytest.mark.parametrize("what", ["y", "fx", "k", "se-diag", "se-full"])
def test_dropped_rows_equal_rows_deleted(gpu_ctx, what):
    nlev, nblk, m, nprof = 65, 2, 98, 4
    base, gammas, _ = seeded(nlev, nblk, m, what == "se-full", False, nprof)
    gamma = gammas[0]
    clean = Dev(base, gamma).run(gpu_ctx)
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
        lin, sol, cost = reference(case, gamma)
        shared = what.startswith("se")
        assert sol["nobs"].tolist() == ([m - 1] * nprof if shared else [m, m - 1, m, m])
        got = Dev(case, gamma).run(gpu_ctx)
        check_prepare(got, lin, (what, row))
        check_solve(got, sol, case, (what, row))
        check_cost(got, cost, (what, row))
        if not shared:                                         # the neighbours never see it: bit for bit
            for i in (0, 2, 3):
                for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
                    assert np.array_equal(got[key][i], clean[key][i]), (what, row, i, key)


@pytest.mark.parametrize("pattern", list(oer.SEAM_DROPS))
@pytest.mark.parametrize("what", ["y", "k"])
def test_dropped_rows_at_the_seams_equal_rows_deleted(gpu_ctx, what, pattern):
    """m = 65: row 64 is the only row of the third tile of k_lm_prepare<3> and the only entry of the second register of
    k_lm_solve's wave 0.  Profile 1 (gamma = 0.25) loses the last row of a tile, the first of the next, a whole tile, or
    every row but 64."""
    (nlev, nblk, m), nprof = oer.SEAM_SHAPE, 4
    dropped = oer.SEAM_DROPS[pattern]
    base, gammas, _ = seeded(nlev, nblk, m, False, False, nprof)
    gamma = gammas[0]
    clean = Dev(base, gamma).run(gpu_ctx)
    case = oer.drop_rows(base, what, dropped, 1)
    lin, sol, cost = reference(case, gamma)
    assert sol["nobs"].tolist() == [m, m - len(dropped), m, m]
    got = Dev(case, gamma).run(gpu_ctx)
    check_prepare(got, lin, (what, pattern))
    check_solve(got, sol, case, (what, pattern))
    check_cost(got, cost, (what, pattern))
    alone = oer.one_profile(dict(x_new=got["x_new"], chi2=got["chi2"]), 1)
    print((what, pattern), "profile 1 alone", oer.block_errors(alone, oer.one_profile(sol, 1), case))
    for i in (0, 2, 3):                                       # the neighbours never see it: bit for bit
        for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (what, pattern, i, key)


def test_status_values_and_untouched_neighbours(gpu_ctx):
    nlev, nblk, m, nprof = 65, 2, 98, 7
    base = oer.make_case(nlev, nblk, m, nprof=nprof, xa_per_profile=True)
    gamma = np.array([0.0, 1.0, 4.0, 1.0, 0.25, -1.0, 1e3])
    clean = Dev(base, np.abs(gamma)).run(gpu_ctx)
    case = _copy(base)
    for b in case["k"]:
        b[1] = np.nan                                          # what an invalid profile of the Jacobian call looks like
    case["fx"][1] = np.nan
    case["x"][3, 1, 17] = np.nan
    d = Dev(case, gamma)
    got = d.run(gpu_ctx)
    lin, sol, cost = reference(case, gamma)
    assert got["lin_status"].tolist() == lin["lin_status"].tolist() == [1, 3, 1, 0, 1, 1, 1]
    assert got["status"].tolist() == sol["status"].tolist() == [1, 3, 1, 0, 1, 2, 1]
    assert got["nobs"].tolist() == [m, 0, m, 0, m, m, m]
    # nothing observed: the damped pull towards the prior alone; G0, r, K dx and keep 0; the cost is its prior term
    assert np.array_equal(got["x_new"][1], case["xa"][1] + 0.5 * (case["x"][1] - case["xa"][1])) and got["chi2"][1] == 0.0
    assert not got["g0"][1].any() and not got["r"][1].any() and not got["kdx"][1].any() and not got["keep"][1].any()
    assert got["cost_obs"][1] == 0.0 and got["cost"][1] == got["cost_prior"][1] > 0.0 and got["cost_status"][1] == 1
    # the state not finite: NaN from prepare and solve, +inf from the cost
    assert np.isnan(got["x_new"][3]).all() and np.isnan(got["chi2"][3]) and np.isnan(got["r"][3]).all()
    assert np.isnan(got["kdx"][3]).all() and np.isnan(got["g0"][3]).all() and not got["keep"][3].any()
    assert np.isposinf([got["cost"][3], got["cost_obs"][3], got["cost_prior"][3]]).all() and got["cost_status"][3] == 1
    # a negative gamma: NaN from the solve alone
    assert np.isnan(got["x_new"][5]).all() and np.isnan(got["chi2"][5])
    for i in (0, 2, 4, 6):
        for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (i, key)
    for key in LIN_KEYS + COST_KEYS:
        assert np.array_equal(got[key][5], clean[key][5]), key
    for g in (np.inf, np.nan):
        d = Dev(base, np.where(np.arange(nprof) == 2, g, 1.0))
        assert d.run(gpu_ctx)["status"].tolist() == [1, 1, 2, 1, 1, 1, 1]
    # NaN in xa alone is status 0 as well
    case = _copy(base)
    case["xa"][2, 0, 64] = np.inf
    got = Dev(case, 1.0).run(gpu_ctx)
    assert got["lin_status"].tolist() == [1, 1, 0, 1, 1, 1, 1] == got["status"].tolist() and np.isnan(got["x_new"][2]).all()
    # an indefinite G (a negative variance larger than K Sa K^T's diagonal) and with it an indefinite Se
    case = _copy(base)
    case["se"][40] = -1e9
    got = Dev(case, 1.0).run(gpu_ctx)
    assert got["lin_status"].tolist() == [1] * nprof and got["status"].tolist() == [2] * nprof == got["cost_status"].tolist()
    assert got["nobs"].tolist() == [m] * nprof and np.isnan(got["x_new"]).all() and np.isnan(got["chi2"]).all()
    assert np.isnan(got["cost"]).all() and np.isnan(got["cost_obs"]).all() and np.isnan(got["cost_prior"]).all()
    # a trial whose forward run failed in a kept row: +inf, to be rejected; in a dropped row it is not looked at
    d = Dev(base, 1.0)
    first = d.run(gpu_ctx)
    d.fx[2, 7] = float("nan")
    d.out["keep"][4, 11] = 0
    d.fx[4, 11] = float("inf")
    gpu_ctx.oe_cost_device(**d.cost_args())
    torch.cuda.synchronize()
    again = d.host()
    assert np.isposinf(again["cost"][2]) and np.isposinf(again["cost_obs"][2]) and again["cost_status"][2] == 1
    assert np.isfinite(again["cost"][4]) and again["cost"][4] < first["cost"][4] and again["cost_prior"][4] == first["cost_prior"][4]
    for i in (0, 1, 3, 5, 6):
        assert again["cost"][i] == first["cost"][i]


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_inactive_profiles_keep_their_sentinels(gpu_ctx, se_full):
    case, gammas, _ = seeded(65, 2, 98, se_full, False, 4)
    full = Dev(case, gammas[0]).run(gpu_ctx)
    d = Dev(case, gammas[0])
    blank = d.host()
    active = _dev(np.array([1, 0, 1, 0], dtype=np.uint8))
    got = d.run(gpu_ctx, active)
    for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
        for i in (0, 2):
            assert np.array_equal(got[key][i], full[key][i]), (key, i)
        for i in (1, 3):
            assert np.array_equal(got[key][i], blank[key][i]), (key, i)


def test_outputs_do_not_depend_on_the_batch(gpu_ctx):
    nlev, nblk, m = 65, 2, 98
    big = oer.make_case(nlev, nblk, m, nprof=300)
    gamma = np.resize(np.array(lmr.GAMMAS), 300)
    got300 = Dev(big, gamma).run(gpu_ctx)
    again = Dev(big, gamma).run(gpu_ctx)
    keys = LIN_KEYS + SOLVE_KEYS + COST_KEYS
    for key in keys:
        assert np.array_equal(got300[key], again[key], equal_nan=True), key
    assert (got300["status"] == 1).all() and (got300["lin_status"] == 1).all() and (got300["cost_status"] == 1).all()

    def sub(lo, hi):
        part = dict(big, k=[b[lo:hi] for b in big["k"]], x=big["x"][lo:hi], y=big["y"][lo:hi], fx=big["fx"][lo:hi])
        return Dev(part, gamma[lo:hi]).run(gpu_ctx)

    for nprof in (1, 5):
        got = sub(0, nprof)
        for key in keys:
            assert np.array_equal(got[key], got300[key][:nprof]), (nprof, key)
    got = sub(299, 300)                                                  # the last profile of the large batch as a batch of one
    for key in keys:
        assert np.array_equal(got[key][0], got300[key][299]), key


def test_repeat_calls_allocate_nothing_and_order_on_the_callers_stream(gpu_ctx):
    case, gammas, _ = seeded(180, 2, 98, False, False, 3)
    first = Dev(case, gammas[0]).run(gpu_ctx)
    d = Dev(case, gammas[0])
    side = torch.cuda.Stream()
    doubled, summed = torch.empty_like(d.out["x_new"]), torch.empty_like(d.out["cost"])

    def calls():
        gpu_ctx.oe_lm_prepare_device(**d.prepare_args(stream=side.cuda_stream))
        gpu_ctx.oe_lm_solve_device(**d.solve_args(stream=side.cuda_stream))
        gpu_ctx.oe_cost_device(**d.cost_args(stream=side.cuda_stream))

    with torch.cuda.stream(side):                                    # warm-up of everything this test launches on `side`
        calls()
        torch.mul(d.out["x_new"], 2.0, out=doubled)
        torch.add(d.out["cost"], 1.0, out=summed)
        d.out["x_new"].fill_(-7.0)
        d.out["cost"].fill_(-7.0)
        d.out["g0"].fill_(-7.0)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    calls()
    side.synchronize()
    assert torch.cuda.mem_get_info()[0] == before                    # hipMemGetInfo: the calls took and freed nothing
    with torch.cuda.stream(side):
        d.out["x_new"].fill_(-7.0)
        d.out["cost"].fill_(-7.0)
        d.out["g0"].fill_(-7.0)                                      # the solve reads what prepare writes: ordered behind it
        calls()
        torch.mul(d.out["x_new"], 2.0, out=doubled)                  # consumed on the same stream: ordered behind the kernels
        torch.add(d.out["cost"], 1.0, out=summed)
    side.synchronize()                                               # that stream alone, no device-wide wait
    assert np.array_equal(doubled.cpu().numpy(), 2.0 * first["x_new"])
    assert np.array_equal(summed.cpu().numpy(), first["cost"] + 1.0)
    assert d.out["status"].cpu().tolist() == [1] * 3


def test_argument_refusals(gpu_ctx):
    case = oer.make_case(3, 3, 14, nprof=2)
    d = Dev(case, 1.0)
    rec = _native.MwrtOeLm

    def code(entry, base, **change):
        with pytest.raises(MwrtError) as ei:
            getattr(gpu_ctx, entry)(**dict(base, **change))
        return ei.value.code, str(ei.value)

    required = dict(
        oe_lm_prepare_device=("d_x", "d_xa", "d_sa", "d_se", "d_y", "d_fx", "d_g0", "d_r", "d_kdx", "d_keep", "d_lin_status"),
        oe_lm_solve_device=("d_x", "d_xa", "d_sa", "d_se", "d_gamma", "d_g0", "d_r", "d_kdx", "d_keep", "d_lin_status", "d_x_new",
                            "d_status"),
        oe_cost_device=("d_x", "d_xa", "d_se", "d_y", "d_fx", "d_keep", "d_sa_inv", "d_cost"))
    for entry, base in (("oe_lm_prepare_device", d.prepare_args()), ("oe_lm_solve_device", d.solve_args()),
                        ("oe_cost_device", d.cost_args())):
        getattr(gpu_ctx, entry)(**base)                                  # the unchanged call is accepted
        for name in required[entry]:
            assert code(entry, base, **{name: None})[0] == -1, (entry, name)
        if entry == "oe_cost_device":
            assert code(entry, base, nblk=0)[0] == -1 and code(entry, base, nblk=5)[0] == -1
        else:
            k = base["d_k"]
            assert code(entry, base, d_k=[k[0], None, k[2]])[0] == -1
            assert code(entry, base, d_k=[])[0] == -1 and code(entry, base, d_k=[k[0]] * 5)[0] == -1
        assert code(entry, base, reserved=1)[0] == -1
        assert code(entry, base, nlev=0)[0] == -1 and code(entry, base, m=0)[0] == -1 and code(entry, base, nprof=-1)[0] == -1
        assert code(entry, base, struct_size=rec.d_k.offset - 4)[0] == -1 and code(entry, base, struct_size=0)[0] == -1
        assert code(entry, base, struct_size=rec.d_x.offset)[0] == -1    # the record ends before a required pointer: NULL
        c, text = code(entry, base, m=_native.OE_MAX_M + 1)
        assert c == -5 and str(_native.OE_MAX_M) in text
        c, text = code(entry, base, nlev=1025)
        assert c == -5 and "1024" in text
        getattr(gpu_ctx, entry)(**dict(base, nprof=0))                   # nothing to do is not an error
    # optional outputs beyond a shorter record are not written: a solve whose record ends after d_status
    d.reset()
    gpu_ctx.oe_lm_prepare_device(**d.prepare_args())
    gpu_ctx.oe_lm_solve_device(**dict(d.solve_args(), struct_size=rec.d_chi2.offset))
    torch.cuda.synchronize()
    got = d.host()
    assert got["status"].tolist() == [1, 1] and (got["chi2"] == -7.0).all() and (got["nobs"] == -7).all()


# ---- end to end: OneDVar.retrieve_lm on the real operator ----
NPROF, NLEV, NANG, NF = 4, 12, 2, 3
M = NANG * NF


def _retrieval_setup(blocks=("t", "h")):
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    P = pr.synthetic_profiles(NPROF, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, NLEV)).astype(int)           # 12 of the 180 levels, ground to ~12 km
    P = {k: np.ascontiguousarray(v[:, pick]) for k, v in P.items()}
    frq, elev = np.array([22.24, 31.4, 53.86]), np.array([90.0, 19.2])
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 3.0)
    nblk = len(blocks)
    sa = np.zeros((nblk * NLEV, nblk * NLEV))
    for b, sig in enumerate((2.0, 0.1, 0.05)[:nblk]):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig ** 2 * corr
    se = np.full(M, 0.25)
    prior = [t, rh]
    if nblk == 3:
        liq = torch.zeros_like(t)
        liq[:, 2:4] = 0.05                                           # two adjacent cloudy levels [g m-3]
        prior.append(liq)
    prior = torch.stack(prior, dim=1).contiguous()
    ov = retrieval.OneDVar("R24", frq, elev, _dev(sa), _dev(se), variables=JacVariables.of(humidity="rh"), blocks=blocks,
                           xa=prior.clone())
    return ov, z, p, prior, sa, se


def _truth(prior, seed=6):
    rng = np.random.default_rng(seed)
    bump = np.exp(-((np.arange(NLEV) - 3.0) / 4.0) ** 2)             # a smooth departure from the prior
    parts = [3.0 * bump, 0.12 * bump]
    if prior.shape[1] == 3:
        parts.append(np.where((np.arange(NLEV) >= 2) & (np.arange(NLEV) < 4), 0.1, 0.0))
    return prior + _dev(np.stack(parts)[None] * rng.uniform(0.5, 1.0, (NPROF, 1, 1)))


def test_one_retrieve_lm_iteration_equals_the_iteration_assembled_on_the_host(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    ov, z, p, prior, sa, se = _retrieval_setup()
    rng = np.random.default_rng(5)
    x0 = prior + _dev(rng.standard_normal(tuple(prior.shape)) * np.array([0.5, 0.02])[None, :, None])
    y = _dev(250.0 + rng.standard_normal((NPROF, NANG, NF)))
    y[2, 1, 0] = float("nan")                                        # one observation missing
    gamma0 = 0.25
    res = ov.retrieve_lm(z, p, y, x0=x0, max_iter=1, gamma0=gamma0)
    torch.cuda.synchronize()
    # the same iteration from the K-matrix call's outputs with the NumPy reference
    zz, t, rh, _, _ = ov.physical(z, p, x0)
    tb, valid, rows = retrieval._native_k_matrix("R24", zz, p, t, rh, None, None, ov.frq, ov.elev, ov.variables, ("t", "h"), _cur())
    torch.cuda.synchronize()
    assert valid.cpu().tolist() == [1] * NPROF
    case = dict(k=[rows[b].cpu().numpy().reshape(NPROF, M, NLEV) for b in ("t", "h")], x=x0.cpu().numpy(),
                xa=prior.cpu().numpy(), sa=sa, se=se, y=y.cpu().numpy().reshape(NPROF, M), fx=tb.cpu().numpy().reshape(NPROF, M))
    lin, sol, cost = reference(case, gamma0)
    assert sol["status"].tolist() == [1] * NPROF and sol["nobs"].tolist() == [M, M, M - 1, M] and sol["cond"].max() <= oer.COND_MAX
    x_try = ov.clamp(_dev(sol["x_new"]))
    fx_try = ov.forward(z, p, x_try)[0].cpu().numpy().reshape(NPROF, M)
    cost_try = lmr.cost_reference(x_try.cpu().numpy(), case["xa"], se, case["y"], fx_try, lin["keep"], sym_inv(sa))
    accept = cost_try["cost"] <= cost["cost"]
    margin = np.abs(cost_try["cost"] - cost["cost"]) / cost["cost"]
    print("accepted:", accept.tolist(), "J:", cost["cost"].tolist(), "->", cost_try["cost"].tolist())
    assert (margin > 1e-6).all()                                     # no decision of this case hangs on the last bits of J
    want = np.where(accept[:, None, None], x_try.cpu().numpy(), case["x"])
    got = dict(x_new=res.x.cpu().numpy(), chi2=None)
    err = oer.block_errors(got, dict(sol, x_new=want), case)
    print("retrieve_lm, one iteration:", err)
    assert err["x_new"] <= oer.TOL
    assert np.allclose(res.gamma.cpu().numpy(), np.where(accept, gamma0 / 10.0, gamma0 * 10.0), rtol=1e-15, atol=0)
    assert np.allclose(res.cost.cpu().numpy(), np.where(accept, cost_try["cost"], cost["cost"]), rtol=1e-9, atol=0)
    assert res.iterations.cpu().tolist() == [1] * NPROF and res.nobs.cpu().tolist() == [M, M, M - 1, M]


@pytest.mark.parametrize("blocks", [("t", "h"), ("t", "h", "liq")], ids=["clear", "cloudy"])
def test_retrieve_lm_descends_and_closes_on_noise_free_observations(gpu_ctx, blocks):
    ov, z, p, prior, sa, se = _retrieval_setup(blocks)
    x_true = _truth(prior)
    y, valid = ov.forward(z, p, x_true)
    assert valid.cpu().tolist() == [1] * NPROF
    sa_inv, xa = sym_inv(sa), prior.cpu().numpy().reshape(NPROF, -1)

    def residual_rms_and_cost(x):
        """RMS of F(x) - y over the batch and, per profile, J recomputed here from the device's forward run."""
        r = (ov.forward(z, p, x)[0] - y).cpu().numpy().reshape(NPROF, -1)
        dx = x.cpu().numpy().reshape(NPROF, -1) - xa
        return float(np.sqrt((r ** 2).mean())), (r ** 2 / se).sum(axis=1) + np.einsum("ij,jk,ik->i", dx, sa_inv, dx)

    full = ov.retrieve_lm(z, p, y, max_iter=20)
    n_it = int(full.iterations.max())
    print("trials per profile:", full.iterations.cpu().tolist(), "gamma:", full.gamma.cpu().tolist())
    assert full.converged.all() and 2 <= n_it < 20
    rms, cost = (list(v) for v in zip(residual_rms_and_cost(prior)))
    for it in range(1, n_it + 1):                                    # the state after `it` iterations: every accepted state
        res = ov.retrieve_lm(z, p, y, max_iter=it)
        r, j = residual_rms_and_cost(res.x)
        rms.append(r)
        cost.append(j)
    print("TB residual RMS per iteration:", rms)
    print("cost J per iteration and profile:", [c.tolist() for c in cost])
    assert torch.equal(res.x, full.x)
    assert rms[0] > np.sqrt(se[0])                                   # the prior does not already fit
    assert all((b <= a).all() for a, b in zip(cost, cost[1:])), cost
    assert (cost[-1] < cost[0]).all() and np.allclose(full.cost.cpu().numpy(), cost[-1], rtol=1e-9, atol=0)
    assert rms[-1] < np.sqrt(se[0]), rms
    assert (full.status == 1).all() and (full.x[:, 1:] >= 0).all()
    assert (full.dfs > 0).all() and (full.dfs < M).all()
    assert (full.post_var <= _dev(np.diag(sa)).reshape(len(blocks), NLEV)).all()
