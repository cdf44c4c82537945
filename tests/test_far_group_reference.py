"""The running fraction that carries the fused kernel's far-line sums across the quads of a group (far_groups_accumulate,
csrc/mwrt_absorption.hip.h), restated in NumPy (tests/far_group_reference.py) and held against exact rational sums.

Error bars.  Over 10^4 seeded sets (seed 20261019, 1 - 12 quads each, the inputs of random_far_set) the worst error relative
to sum |term_i| was

    against the exact line sum            quad form 4.295e-10   group form 4.295e-10 (5 quads), 4.295e-10 (6)   ratio 1.000
    against the exact sum of the quads    quad form 5.034e-16   group form 8.758e-16 (5 quads), 8.815e-16 (6)   ratio 1.740, 1.751

(the first is the cancellation in u^2 + A2 u + Bc next to a line at 1 THz, shared by both forms; the second is what the forms
do differently).  The bars are twice the worst ratio seen: 2.0 on the first measure, 3.48 (group of 5) and 3.50 (group of 6)
on the second, each applied to what the quad form gives on the same inputs.  The test runs the first 1500 of those sets
(ratios 1.000 and 1.243 / 1.559 there)."""
from fractions import Fraction

import numpy as np
import pytest

import far_group_reference as fg

SEED = 20261019
NSETS = 1500
BAR_LINE_SUM = 2.0
BAR_ACCUMULATION = {fg.FAR_GROUP_QUADS: 3.48, fg.FAR_GROUP_QUADS + 1: 3.50}


@pytest.mark.parametrize("group", [fg.FAR_GROUP_QUADS, fg.FAR_GROUP_QUADS + 1])
def test_group_form_is_as_accurate_as_the_quad_form(group):
    rng = np.random.default_rng(SEED)
    worst = np.zeros(4)
    for _ in range(NSETS):
        u, lines = fg.random_far_set(rng, int(rng.integers(1, 13)))
        worst = np.maximum(worst, fg.errors(u, lines, group))
    eq, eg, aq, ag = worst
    print(f"group of {group}: against the line sum quad {eq:.3e} group {eg:.3e} (ratio {eg / eq:.3f}); "
          f"against the quads' sum quad {aq:.3e} group {ag:.3e} (ratio {ag / aq:.3f})")
    assert eg <= BAR_LINE_SUM * eq
    assert ag <= BAR_ACCUMULATION[group] * aq


def test_inputs_cover_the_admission_limit_and_both_signs():
    rng = np.random.default_rng(SEED)
    closest, signs, centres = np.inf, set(), []
    for _ in range(300):
        u, lines, c = fg.random_far_set(rng, 3, centres=True)
        f = np.sqrt(u)
        assert (np.abs(c - f) >= fg.FAR_MIN_GHZ * (1 - 1e-9)).all() and (c >= 1.0 - 1e-9).all() and (c <= 1000.0 + 1e-9).all()
        closest = min(closest, np.abs(c - f).min())
        signs |= set(np.sign(lines[:, 0])) | set(np.sign(lines[:, 1]))
        centres += list(c)
    assert closest <= 1.05 * fg.FAR_MIN_GHZ and signs == {-1.0, 1.0}
    assert min(centres) < 2.0 and max(centres) > 900.0


def extreme_lines(nquads, large):
    """Lines whose denominators sit at an end of the admissible range: centre 1 THz seen from 1 GHz (1e12 each), or centre
    1 GHz seen from 0.8 GHz at the admission limit with a negligible width (0.04 * 3.24 = 0.13 each, above the 0.04 bound)."""
    n = 4 * nquads
    if large:
        return 1.0, fg.far_lines(np.full(n, 1000.0), np.full(n, 5.0), np.full(n, 1e-3), np.full(n, -1e-3))
    return 0.8 ** 2, fg.far_lines(np.full(n, 1.0), np.full(n, 1e-5), np.full(n, 1e-14), np.full(n, 1e-14))


@pytest.mark.parametrize("large", [False, True])
def test_denominator_stays_inside_its_stated_range(large):
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    u, lines = extreme_lines(fg.FAR_GROUP_QUADS, large)
    trace = []
    s = fg.group_form_sum(u, lines, trace=trace)
    (N, D), = trace
    print(f"{'largest' if large else 'smallest'} denominators, group of {fg.FAR_GROUP_QUADS}: D = {D:.3e}, N = {N:.3e}")
    assert fg.D_MIN <= D <= fg.D_MAX
    assert D * 1e50 < huge and D / 1e50 > tiny and abs(N) * 1e50 < huge and abs(N) / 1e50 > tiny     # the headroom asked for
    t = fg.exact_terms(u, lines)
    assert abs(s - float(sum(t))) <= 1e-14 * float(sum(abs(x) for x in t))
    # one quad more still fits, without the headroom; nine quads in one group do not
    u, lines = extreme_lines(fg.FAR_GROUP_QUADS + 1, large)
    assert np.isfinite(fg.group_form_sum(u, lines, group=fg.FAR_GROUP_QUADS + 1))
    if large:
        u, lines = extreme_lines(9, True)
        assert not np.isfinite(fg.group_form_sum(u, lines, group=9))


@pytest.mark.parametrize("group", [fg.FAR_GROUP_QUADS, fg.FAR_GROUP_QUADS + 1])
def test_a_line_voted_out_changes_nothing_but_the_denominator(group):
    """P = Q = 0 (a line handed to another loop by the wave vote at set-up) stays in its quad: the sum is that of the other
    lines, and D still carries the line's denominator.

    The sum is held to the accumulation's own rounding, not to the front end's cancellation.  With q_k the float64 quotient
    num / den of quad k and V the value N / D carried so far, a later quad computes
        N' = fl(fl(N den) + fl(num D)),  D' = fl(D den)   =>   V' = (V (1 + d1) + q_k (1 + d2)) (1 + d3) / (1 + d4),
    at most 3 u (|V| + |q_k|) <= 3 u sum |q| off the exact V + q_k (u = 2^-53; a group's first quad has two roundings fewer),
    and a group's end adds the division's u |V|.  So against the EXACT sum of the q_k of the same voted lines the form is
    within (3 nq + groups) u sum |q_k| to first order (1 % is allowed for the higher orders): 2.6e-15 for seven quads.  A
    merge that mishandled a zero numerator -- dropped num D, or D's factor -- would be off at the size of a term."""
    rng = np.random.default_rng(SEED + 1)
    u_round = 2.0 ** -53
    worst = 0.0
    for _ in range(200):
        nq = int(rng.integers(1, 8))
        u, lines = fg.random_far_set(rng, nq)
        out = int(rng.integers(0, 4 * nq))
        voted = lines.copy()
        voted[out, :2] = 0.0
        t = fg.exact_terms(u, np.delete(lines, out, axis=0))
        exact, scale = float(sum(t)), float(sum(abs(x) for x in t))
        with_line, without = [], []
        s = fg.group_form_sum(u, voted, group, trace=with_line)
        assert abs(s - exact) <= BAR_LINE_SUM * 4.295e-10 * scale               # the voted-out line adds no term of its own
        acc, qsum = fg.exact_quads_sum(u, voted)
        bar = 1.01 * (3 * nq + len(with_line)) * u_round
        err = float(abs(Fraction(float(s)) - acc) / qsum)
        worst = max(worst, err / bar)
        assert err <= bar                                                        # ... and the merges lose nothing around it
        if nq <= group:                                                          # one group: its D is the product of all
            one = voted.copy()
            one[out, 2:] = [0.0, 1.0 - u * u]                                    # ... and this line's denominator made 1
            fg.group_form_sum(u, one, group, trace=without)
            d_line = u * (u + lines[out, 2]) + lines[out, 3]
            assert np.isclose(with_line[0][1], without[0][1] * d_line, rtol=1e-12)
    print(f"group of {group}: worst accumulation error / bar = {worst:.3f}")
