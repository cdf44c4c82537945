"""The geometry table of the windowed fine-grid path: frequency lists chosen by where they fall relative to the line
centres, shared by tests/test_window_plan.py (CPU: the plan itself), tests/test_window_geometry.py (GPU: the kernels on it)
and tools/window_geometry_errors.py.  ``reaches(case, model, plan)`` states, per case, which bits the dumped plan must
show -- so that a case demonstrably reaches the branch it is in the table for."""
import dataclasses

import numpy as np

import window_reference as wr

CPU_MODELS = ("R98", "R17", "R24")
O2_118, O2_566 = 118.7503, 566.8956
H2O_22, H2O_183, H2O_556 = 22.23508, 183.310087, 556.935985


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    frq: np.ndarray
    gpu_models: tuple = ("R24",)
    eligible: bool = True
    heavy_hpa: float = 0.0          # GPU: profile 1 gets three ground levels at this pressure, 150 K, saturated

    def __str__(self):
        return self.name


def _sd_far_start(model_name="R24"):
    """first whole GHz from which the 22-GHz line's speed-dependent shape cannot reach by the host's bound"""
    from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp
    m = sp.get_model(model_name)
    k = int(np.argmin(np.abs(m.h2o["fl"] - H2O_22)))
    return float(np.ceil(float(m.h2o["fl"][k]) + 10.0 * wr.sd_halfwidth_bound(m, k) + 1.0))


def _build():
    lin = np.linspace
    raised = lin(107.95, 113.95, 128)
    raised[-1] += 1e-9
    gband = np.sort(np.append(lin(180.5, 186.1, 159), H2O_183))
    irregular = np.sort(np.random.default_rng(1).uniform(109.74, 114.74, 128))
    irregular[0], irregular[-1] = 109.74, 114.74
    clustered = np.concatenate([lin(109.74, 109.7401, 100), lin(109.7401, 114.74, 29)[1:]])
    sd0 = _sd_far_start()
    return [
        Case("118-far-below", lin(109.74, 114.74, 128), gpu_models=("R98", "R24")),
        Case("118-near-below", lin(109.76, 114.76, 128)),
        Case("118-far-above", lin(122.76, 127.76, 128)),
        Case("span-limit", lin(107.95, 113.95, 128)),
        Case("span-limit-plus", raised, eligible=False),
        # the 118-GHz line 4.4 GHz beyond a 6-GHz window: far by the 4-GHz floor alone, direct by the 1.6 half-spans
        Case("118-ratio-margin", lin(108.35, 114.35, 128)),
        Case("band-top", lin(68.5, 74.5, 128)),
        Case("g-band-core", gband),
        Case("sdint-at-5-spans", lin(186.86, 192.86, 128)),
        Case("sdint-inside-5-spans", lin(186.86, 192.86, 128) - 0.02),
        Case("sdint-3-ghz", lin(186.30, 188.30, 128)),
        Case("sd-window-far", lin(sd0, sd0 + 5.0, 128)),
        # at 150 K there is next to no vapour, so 2000 hPa of dry air widen the line to 9.2 GHz, short of the host's bound
        # (9.8 GHz: 1100 hPa of air AND 150 hPa of vapour): the line stays in the far set; 2500 hPa reach the window
        Case("sd-heavy-ground-2000", lin(sd0, sd0 + 5.0, 128), heavy_hpa=2000.0),
        Case("sd-taken-back", lin(sd0, sd0 + 5.0, 128), heavy_hpa=2500.0),
        # 26-38 GHz in 200 steps puts 7.66 GHz under the first 128 frequencies: the planner merges it (CPU), the entries
        # refuse it (GPU); the same merge on a list the entries accept is the case after it
        Case("merge-partial", lin(26.0, 38.0, 200), eligible=False),
        Case("merge-partial-eligible", lin(26.0, 35.4, 200)),
        Case("merge-refused", lin(33.0, 45.0, 256)),
        Case("two-frequency-tail", lin(20.0, 25.16, 130)),
        Case("two-frequency-tail-unmerged", lin(52.0, 57.16, 130)),
        Case("one-frequency-tail", lin(20.0, 25.16, 130)[:129], eligible=False),
        Case("cutoff-crossing", lin(564.2, 569.2, 128)),
        Case("cutoff-guard-inside", lin(570.0, 575.0, 128)),
        Case("cutoff-guard-out", lin(571.70, 576.70, 128)),
        Case("irregular", irregular),
        Case("clustered", clustered),
        Case("tight", 57.6 + 1e-9 * np.arange(256)),
    ]


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def line_bit(table, centre):
    """bit of the line at `centre` GHz in a table of line centres, or 0 where the model has no such line"""
    d = np.abs(np.asarray(table) - centre)
    return 1 << int(np.argmin(d)) if d.min() < 1e-3 else 0


def reaches(case, m, plan):
    """assert the bits of `plan` (wr.plan_arrays of the dump, model `m`) that put `case` on its branch"""
    wins, masks, name = plan["windows"], plan["masks"], case.name
    o2 = lambda c: line_bit(m.o2["f"], c)
    h2o = lambda c: line_bit(m.h2o["fl"], c)
    grid = sorted(wins, key=lambda w: w["first_chunk"])
    sd_model = bool((m.h2o["w2"] > 0).any())
    far_h = lambda w: w["h2o_far_both"] | w["h2o_far_res"]
    if name in ("118-far-below", "118-far-above", "span-limit", "irregular", "clustered"):
        assert len(wins) == 1 and wins[0]["o2_far"] & o2(O2_118)
        assert wins[0]["o2_far"] == (1 << m.n_o2) - 1                   # ... and every other line: the 118 line is the nearest
    if name == "118-near-below":
        far = BY_NAME["118-far-below"]
        assert wins[0]["o2_far"] == ((1 << m.n_o2) - 1) ^ o2(O2_118), "one bit against %s" % far.name
    if name == "118-ratio-margin":
        assert wins[0]["o2_far"] == ((1 << m.n_o2) - 1) ^ o2(O2_118) and 4.0 < O2_118 - wins[0]["fhi"] < 1.6 * 3.0
    if name in ("span-limit", "span-limit-plus"):
        assert (wins[0]["fhi"] - wins[0]["flo"] == 6.0) == (name == "span-limit")
        assert 118.7503 - wins[0]["fhi"] > 4.8 or name != "span-limit"
    if name == "band-top":
        assert bin(wins[0]["o2_far"]).count("1") == {40: 32, 49: 39}[m.n_o2]     # the band's upper wing (8 / 10 lines) direct
    if name == "g-band-core":
        # 128 + 32 frequencies; no oxygen line is near and the water far sets agree, so the rule merges them
        assert [w["nchunks"] for w in grid] == [10] and H2O_183 in plan["frq"] and grid[0]["flo"] < H2O_183 < grid[0]["fhi"]
        assert all(not far_h(w) & h2o(H2O_183) for w in wins)
        k = h2o(H2O_183)
        assert all(not mk["h2o_sdint"] & k and not mk["h2o_sdfar"] & k for mk in masks[:8])
        assert not sd_model or all(mk["h2o_sd"] & k for mk in masks)
    if name.startswith("sdint") and sd_model:
        k = h2o(H2O_183)
        first = bool(masks[0]["h2o_sdint"] & k)
        assert first == (name == "sdint-at-5-spans"), name
        assert masks[1]["h2o_sdint"] & k
        f = plan["frq"]
        dmin, span = f[0] - H2O_183, f[15] - f[0]
        if name == "sdint-3-ghz":
            assert dmin < 3.0 and dmin >= 5.0 * span                      # the 3-GHz limb alone says no
        else:
            assert dmin >= 3.0 and abs(dmin / span - 5.0) < 0.03          # the 5-span limb decides
    if name.startswith("sd-") and sd_model:
        assert wins[0]["h2o_far_both"] & h2o(H2O_22)                      # a speed-dependent line in the window's far set
        assert not far_h(wins[0]) & h2o(H2O_183)
    if name.startswith("merge-partial"):
        assert [(w["first_chunk"], w["nchunks"]) for w in grid] == [(0, 13)]
        assert len(plan["frq"]) % 16 == 8
    if name == "merge-refused":
        assert [(w["first_chunk"], w["nchunks"]) for w in grid] == [(0, 8), (8, 8)]
        half = 0.5 * (plan["frq"][-1] - plan["frq"][0])
        assert 50.4742 - plan["frq"][-1] < 1.6 * half and all(w["o2_far"] == (1 << m.n_o2) - 1 for w in wins)
    if name == "two-frequency-tail":                                      # out of band: the tail joins the window before it
        assert [(w["first_chunk"], w["nchunks"]) for w in grid] == [(0, 9)] and len(plan["frq"]) == 130
    if name == "two-frequency-tail-unmerged":                             # oxygen lines near: a window of two targets
        assert [(w["first_chunk"], w["nchunks"]) for w in grid] == [(0, 8), (8, 1)] and len(plan["frq"]) == 130
        assert grid[1]["flo"] == plan["frq"][128] and grid[1]["fhi"] == plan["frq"][129]
    if name == "one-frequency-tail":
        assert len(plan["frq"]) == 129
    if name == "cutoff-crossing":
        assert not far_h(wins[0]) & h2o(H2O_183) and not far_h(wins[0]) & h2o(H2O_556)
        assert not wins[0]["o2_far"] & o2(O2_566)
        assert plan["frq"][0] + H2O_183 < 750.0 < plan["frq"][-1] + H2O_183
    if name == "cutoff-guard-inside":
        assert not far_h(wins[0]) & h2o(H2O_183) and 750.0 < plan["frq"][0] + H2O_183 < 755.0
    if name == "cutoff-guard-out":
        assert wins[0]["h2o_far_res"] & h2o(H2O_183) and not wins[0]["h2o_far_both"] & h2o(H2O_183)
    if name == "tight":
        assert len(wins) == 2 and all(len(set(w["fnode"])) == 16 and len(set(w["fnode_h"])) == 8 for w in wins)
        assert plan["frq"][-1] - plan["frq"][0] < 2.6e-7


def heavy_ground(P, hpa):
    """profile 1 with its lowest three levels at `hpa`, 150 K, saturated: at or beyond the edge of the atmospheres the host's
    half-width bound covers"""
    P = {k: v.copy() for k, v in P.items()}
    if hpa:
        P["p"][1, :3], P["t"][1, :3], P["rh"][1, :3] = hpa, 150.0, 1.0
    return P
