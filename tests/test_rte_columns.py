"""k_rte_tau and the K2 passes of k_tb_fused on the hand-built columns of tests/rte_cases.py, against the long-double reference
of tests/rte_reference.py under bars derived there (never the project's 1e-6 K), plus the properties that hold bit for bit.
Every case is compared in full: the only outputs left out of a comparison are those that are NaN by contract, which are
asserted to be NaN and counted.  The figures each test prints are those tools/rte_column_errors.py writes to
profiles/rte_column_errors.json.

Measured on the MI355X (worst error / bar over the table): k_rte_tau 0.86 (9.3e-12 K on 20 - 60 GHz columns, 1.8e-10 K on the
1 - 1000 GHz grids), the K2 passes of k_tb_fused 0.56 (8.7e-12 K); every exact property holds with 0 differing values."""
import numpy as np
import pytest

import rte_cases as rc
import rte_device as rd

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_every_case_is_held():
    held = set(rd.CHECKS)
    assert held == set(rc.names(held=True)) and set(rc.table()) - held == {"inf_tau"}


@pytest.mark.parametrize("name", sorted(rd.CHECKS))
def test_columns_meet_their_bars(gpu_ctx, name):
    for row in rd.CHECKS[name](gpu_ctx):
        assert row["left_out"] == 0 and row["worst_err_over_bar"] <= 1.0, row


@pytest.mark.parametrize("k", range(len(rc.exact_pairs())))
def test_exact_properties(gpu_ctx, k):
    label, na, ia, nb, ib = rc.exact_pairs()[k]
    a, b = rd.cached_run(gpu_ctx, na)[0][ia], rd.cached_run(gpu_ctx, nb)[0][ib]
    assert a.shape == b.shape and a.size > 0
    same = bits(a) == bits(b)
    print("%s: %d values, %d differ" % (label, a.size, (~same).sum()))
    assert np.isfinite(b).all() and same.all(), label


def test_infinite_tau_stays_in_its_column(gpu_ctx):
    """tau = +inf is outside the specified range (include/mwrt.h): only confinement is asserted (the pairs of `inf_tau` above)
    and that the flags the entry reads are not touched"""
    tb, valid = rd.cached_run(gpu_ctx, "inf_tau")
    assert np.array_equal(valid, rc.table()["inf_tau"].valid)
    assert tb.shape == (2, 3, 14) and not (tb == -777.0).any()


def test_a_wave_past_the_last_frequency_writes_nothing(gpu_ctx):
    """nf = 257 starts a second workgroup row whose waves 1-3 hold no frequency; nf = 65 a wave whose lanes 1-63 are idle:
    the runner's output is exactly nf wide per row, so a stray store would land in the next row and break its bar -- and
    every value is written (none keeps the fill)"""
    for name in ("seam_L257_F257", "seam_L10_F65", "odd_lane_257"):
        tb, _ = rd.cached_run(gpu_ctx, name)
        assert not (tb == -777.0).any(), name
