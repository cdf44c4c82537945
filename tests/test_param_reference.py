"""The exact reference of the spectroscopic-parameter Jacobian (tests/param_reference.py: torch autograd of the oracle's
formulas with table entries as leaves) against central differences of the NumPy oracle on deep-copied tables.  No GPU.

The bar is the step error of the quotient: a relative step h = 1e-4 leaves h^2 |f'''| / 6 ~ 1e-8 relative, inside 1e-5 of a
column's largest entry.  The quotient also carries the oracle's own rounding, ~5e-13 K in a TB, divided by the step: where
the step moves no TB by 1e-6 K (h |b| max|column| < 1e-6 K: a weak line seen from these eight frequencies, or a tiny table
entry such as dnu0 = -2.8e-4) that rounding alone is 2.5e-7 .. 3e-3 of the column (measured: error proportional to 1 / h),
so those columns are differenced with h = 1e-2 instead (truncation ~2e-5 (b^2 f''' / f'), measured <= 1.1e-6) -- the bar
stays 1e-5 for every column.  A column that even the larger step moves by less than 1e-6 K (the 987.9-GHz and 1.8-THz
lines seen from below 200 GHz) has no quotient to compare with: it is listed, not compared here, and the device test
compares it with the autograd column like every other."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lbl_oracle as lo  # noqa: E402
import param_reference as prf  # noqa: E402
from test_tl_oracle import CASES, edge_profile, tables_and_frq  # noqa: E402

ANG = np.array([90.0, 30.0, 4.2])
STEP = 1e-4
STEP_WEAK = 1e-2        # where STEP moves no TB by MOVE_MIN (module docstring)
MOVE_MIN = 1e-6         # K
TOL = 1e-5


def case_setup(case):
    m, frq = tables_and_frq(case)
    # eight: line centres, 60 GHz, 2.5 GHz, the pair at the 22-GHz line's cutoff, the SD-window point (without one: 999 GHz)
    frq = frq[[1, 2, 3, 4, 0, 6, 7, 8 if len(frq) == 9 else 5]]
    params = prf.test_params(m)
    return m, frq, params


_cache = {}


def reference(case):
    if case not in _cache:
        m, frq, params = case_setup(case)
        z, p, t, rh = edge_profile()
        _cache[case] = (m, frq, params, (z, p, t, rh), prf.param_jacobian(m, z, p, t, rh, frq, ANG, params))
    return _cache[case]


def oracle_tb(m, prof, frq):
    return lo.tb_cloud_rte(m, *prof, frq, ANG)["tbtotal"].reshape(len(ANG), len(frq))


@pytest.mark.parametrize("case", CASES)
def test_autograd_columns_equal_central_differences_of_the_oracle(case):
    m, frq, params, prof, (tb, kb) = reference(case)
    assert np.abs(tb - oracle_tb(m, prof, frq)).max() <= 1e-12 * np.abs(tb).max()
    worst, skipped = 0.0, []
    for q, (name, line) in enumerate(params):
        b = prf.table_value(m, name, line)
        col = kb[:, :, q]
        if b == 0.0:                                         # no relative step exists: nothing to difference
            continue
        h = STEP if STEP * abs(b) * np.abs(col).max() >= MOVE_MIN else STEP_WEAK
        if h * abs(b) * np.abs(col).max() < MOVE_MIN:        # no step of either size shows in the TBs: nothing to difference
            skipped.append((name, line))
            continue
        fd = (oracle_tb(prf.perturbed_tables(m, name, line, 1.0 + h), prof, frq) -
              oracle_tb(prf.perturbed_tables(m, name, line, 1.0 - h), prof, frq)) / (2.0 * h * b)
        scale = max(np.abs(col).max(), np.abs(fd).max())
        if scale == 0.0:
            continue
        err = np.abs(col - fd).max() / scale
        worst = max(worst, err)
        assert err <= TOL, (case, name, line, err)
    # what cannot be differenced: far lines' columns and tiny entries (shifts, dnu, g); never a scalar, a strength or a width
    # of a first line, and never most of the list
    strong = {"h2o_s1", "h2o_w0", "h2o_w0s", "o2_s300", "o2_w300", "o2_y0"}
    assert not [q for q in skipped if (q[0] in strong and q[1] <= 0) or q[0] in list(prf.PARAM_FIELDS)[:7]], skipped
    assert len(skipped) <= len(params) // 2, skipped
    print(f"{case}: worst column error {worst:.2e} of the column's largest entry; not differenced: {skipped}")


@pytest.mark.parametrize("case", CASES)
def test_unread_parameters_have_exactly_zero_columns(case):
    m, frq, params, prof, (tb, kb) = reference(case)
    for q, (name, line) in enumerate(params):
        unread = (m.h2o_shift_mode == 0 and name in ("h2o_sh", "h2o_shs")) or \
                 (m.o2_mix_mode == 0 and name in ("o2_g0", "o2_g1", "o2_dnu0", "o2_dnu1"))
        if unread:
            assert (kb[:, :, q] == 0.0).all(), (case, name, line)
        elif line >= 0 and prf.table_value(m, name, line) != 0.0 and name not in ("h2o_sh", "h2o_shs"):
            assert np.abs(kb[:, :, q]).max() > 0.0, (case, name, line)


@pytest.mark.parametrize("case", ["R17", "R20SD", "fuzz2"])
def test_all_lines_is_the_weighted_sum_of_the_line_columns(case):
    m, frq = tables_and_frq(case)
    frq = frq[[1, 3, 4]]
    z, p, t, rh = edge_profile()
    for name, n in (("h2o_w0", len(m.h2o["fl"])), ("o2_w300", len(m.o2["f"])), ("o2_y0", len(m.o2["f"]))):
        params = [(name, -1)] + [(name, k) for k in range(n)]
        _, kb = prf.param_jacobian(m, z, p, t, rh, frq, ANG, params)
        b = np.array([prf.table_value(m, name, k) for k in range(n)])
        want = (kb[:, :, 1:] * b).sum(axis=-1)
        assert np.abs(kb[:, :, 0] - want).max() <= 1e-12 * np.abs(kb[:, :, 1:] * b).sum(axis=-1).max() + \
            1e-13 * np.abs(kb[:, :, 1:] * b).max(), (case, name)
