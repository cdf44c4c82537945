"""The windowed fine-grid kernels (k_absorb_win, then k_rte_tau) where the geometry is worst: the table of
tests/window_cases.py -- a strong line just beyond the far margin, the 6-GHz span limit, the 183-GHz speed-dependent line
inside a window, the 750-GHz cutoff crossing a window, merges made and refused, short tails, irregular, clustered and
tight lists -- on three 180-level profiles with their sharp-line top levels.  tests/test_window_plan.py shows on the CPU
that each case's plan reaches its branch; here the kernels run on that plan.

Bars: absorption against lbl_oracle at every frequency 1e-9 relative, windowed and every-line alike (so a failure names
the kernel); windowed against every-line within the plan's own truncation (tests/window_reference.py, from the oracle's
formulas alone) plus 2e-10 for rounding; TB against the oracle 1e-6 K, against the every-line call 1e-8 K.

Measured (tools/window_geometry_errors.py -> profiles/window_geometry_errors.json, quoted in DESIGN.md 4.3): windowed
against the oracle <= 3.0e-10, against every-line <= 3.1e-10 (118-far-above), TB <= 1.4e-9 K."""
import pytest

from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp
from plan_dump_tool import plan_dump_plain, request          # noqa: F401 (the fixture: the planning unit, no sanitisers here)
import window_cases as wc
import window_device as wd
import window_reference as wr

TOL_K = 1e-6                  # TB against the oracle (tests/test_gpu_parity.py)
TOL_REL = 1e-9                # absorption against the oracle
ROUNDING = 2e-10              # windowed against every-line beyond the plan's truncation
PLAN_BAR = 5e-10              # what the plan alone may leave (tests/test_window_plan.py): half of TOL_REL
ERR_UNSUPPORTED = -5

RUNS = [(c, mn) for c in wc.CASES if c.eligible for mn in c.gpu_models]
REFUSED = [c for c in wc.CASES if not c.eligible]


@pytest.fixture(scope="module")
def plans(plan_dump_plain, tmp_path_factory):
    out = {}
    for mn in sorted({mn for _, mn in RUNS}):
        path = tmp_path_factory.mktemp("desc") / (mn + ".desc")
        path.write_bytes(bytes(sp.get_model(mn).to_c()))
        cases = [c for c, x in RUNS if x == mn]
        got = plan_dump_plain([request("tables", path)] + [request("windows", *c.frq) for c in cases])
        out.update({(c.name, mn): wr.plan_arrays(d, c.frq) for c, d in zip(cases, got[1:])})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case, model", RUNS, ids=lambda x: str(x))
def test_kernels_on_the_geometry(gpu_ctx, plans, case, model):
    r = wd.measure(gpu_ctx, case, model, plans[case.name, model])
    print("\n%s %s: windowed vs oracle %.2e, every-line vs oracle %.2e, TB vs oracle %.2e K, vs every-line %.2e K"
          % (case.name, model, r["win_vs_oracle"], r["every_vs_oracle"], r["tb_vs_oracle"], r["tb_vs_every"]))
    for j, (t, d) in enumerate(zip(r["truncation"], r["win_vs_every"])):
        print("  profile %d: windowed vs every-line dry %.2e (plan %.2e) wet %.2e (plan %.2e + %.2e)"
              % (j, d["dry"], t["dry"], d["wet"], t["wet"], t["sd"]))
    assert r["finite"] and r["tb_finite"] and r["valid"]
    # absorption: the project's bar, for both kernels
    assert r["every_vs_oracle"] <= TOL_REL, "every-line kernel"
    assert r["win_vs_oracle"] <= TOL_REL, "windowed kernel"
    # windowed against every-line: what the plan leaves (reference only, itself under half the absorption bar at every
    # level) + rounding
    for j, (t, d) in enumerate(zip(r["truncation"], r["win_vs_every"])):
        assert max(t.values()) <= PLAN_BAR, (j, t)
        assert d["dry"] <= t["dry"] + ROUNDING, (j, d, t)
        assert d["wet"] <= t["wet"] + t["sd"] + ROUNDING, (j, d, t)
    # TB through the automatic path
    assert r["tb_vs_oracle"] <= TOL_K
    assert r["tb_vs_every"] <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("case", REFUSED, ids=str)
def test_ineligible_lists_are_served_by_every_line(gpu_ctx, case):
    r = wd.refusal(gpu_ctx, case, "R24")
    assert r["mode0_is_mode1"]
    assert r["mode2_code"] == ERR_UNSUPPORTED
