"""NumPy restatement, in float64, of how the fused kernel sums its far lines (csrc/mwrt_absorption.hip.h): a far line's two
Lorentz terms are one rational function of u = f^2,

    term = (u P + Q) / (u^2 + A2 u + Bc),      A2 = 2 (w^2 - c^2),   Bc = (c^2 + w^2)^2,

four lines share one quotient num / den (far_quad_terms), and

  * the QUAD form (far_quad_accumulate) adds num / den to a plain sum quad by quad;
  * the GROUP form (far_groups_accumulate) carries the sum across the quads of a group as a fraction N / D,
        first quad   N = S den + num,      D = den
        later quads  N = N den + num D,    D = D den
        group end    S = N / D,
    one division per FAR_GROUP_QUADS quads.

No fused multiply-add and an exact division here (the device has both the other way round): the restatement is about the
algebra -- how rounding errors and magnitudes behave when the sum rides in a fraction -- not about the device's last bit.
``exact_sum`` is the same sum in rational arithmetic over the same float64 inputs."""
from fractions import Fraction

import numpy as np

FAR_GROUP_QUADS = 5               # csrc/mwrt_absorption.hip.h
FAR_MIN_GHZ = 0.2                 # csrc/mwrt_plan.h: the closest a far line's centre comes to a chunk frequency, shift included
D_MIN, D_MAX = 1e-28, 1e241       # the range of D stated next to FAR_GROUP_QUADS


def far_lines(c, w, p, q):
    """(P, Q, A2, Bc) rows from centre c, half width w and numerator n(u) = u p + q (c^2 + w^2)."""
    c, w, p, q = (np.asarray(x, dtype=np.float64) for x in (c, w, p, q))
    cc = c * c + w * w
    return np.stack([p, q * cc, 2.0 * (w * w - c * c), cc * cc], axis=-1)


def quad_terms(u, lines4):
    """num, den of four lines at u = f^2 (far_quad_terms, operation by operation)."""
    P, Q, A2, Bc = (lines4[:, k] for k in range(4))
    d = u * (u + A2) + Bc
    n = u * P + Q
    p01, p23 = d[0] * d[1], d[2] * d[3]
    m01 = n[0] * d[1] + n[1] * d[0]
    m23 = n[2] * d[3] + n[3] * d[2]
    return m01 * p23 + m23 * p01, p01 * p23


def quad_form_sum(u, lines):
    s = np.float64(0.0)
    for k in range(0, len(lines), 4):
        num, den = quad_terms(u, lines[k:k + 4])
        s = s + num / den
    return s


def group_form_sum(u, lines, group=FAR_GROUP_QUADS, trace=None):
    """The running fraction; ``trace`` (a list) receives every (N, D) a group ends with."""
    s = np.float64(0.0)
    nquads = len(lines) // 4
    k = 0
    with np.errstate(over="ignore", invalid="ignore"):
        while k < nquads:
            num, den = quad_terms(u, lines[4 * k:4 * k + 4])
            N, D = s * den + num, den
            k += 1
            for _ in range(1, group):
                if k == nquads:
                    break
                num, den = quad_terms(u, lines[4 * k:4 * k + 4])
                N, D = N * den + num * D, D * den
                k += 1
            if trace is not None:
                trace.append((N, D))
            s = N / D
    return s


def exact_terms(u, lines):
    u = Fraction(float(u))
    out = []
    for P, Q, A2, Bc in lines:
        out.append((u * Fraction(float(P)) + Fraction(float(Q))) / (u * (u + Fraction(float(A2))) + Fraction(float(Bc))))
    return out


def exact_quads_sum(u, lines):
    """The exact sum of the float64 quotients num / den of the quads, and the sum of their magnitudes: what an accumulation
    without rounding would give from the front end's own output."""
    q = [Fraction(float(num)) / Fraction(float(den)) for num, den in (quad_terms(u, lines[k:k + 4]) for k in range(0, len(lines), 4))]
    return sum(q), sum(abs(x) for x in q)


def random_far_set(rng, nquads, centres=False):
    """One frequency and 4 * nquads far lines over the tables' ranges: centres 1 GHz ... 1 THz, detunings from the admission
    limit up, half widths 1e-5 ... 5 GHz, strengths over twelve decades, numerators of both signs.  Returns u = f^2 and the
    lines (and the centres, if asked)."""
    n = 4 * nquads
    f = np.exp(rng.uniform(np.log(1.0), np.log(1000.0)))
    # a third of the lines hug the frequency (detuning 0.2 ... 2 GHz, the first of them at the limit), the rest lie anywhere
    det = np.exp(rng.uniform(np.log(FAR_MIN_GHZ), np.log(2.0), n))
    det[0] = FAR_MIN_GHZ
    near = f + rng.choice([-1.0, 1.0], n) * det
    near = np.where((near < 1.0) | (near > 1000.0), 2.0 * f - near, near)          # mirrored back into the range
    c = np.where(rng.random(n) < 1 / 3, near, np.exp(rng.uniform(np.log(1.0), np.log(1000.0), n)))
    c[0] = near[0]
    c = np.where(np.abs(c - f) < FAR_MIN_GHZ, near, c)
    w = np.exp(rng.uniform(np.log(1e-5), np.log(5.0), n))
    strength = np.exp(rng.uniform(np.log(1e-14), np.log(1e-2), n))
    p = strength * rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 1.0, n)
    q = strength * rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 1.0, n)
    lines = far_lines(c, w, p, q)
    return (f * f, lines, c) if centres else (f * f, lines)


def errors(u, lines, group=FAR_GROUP_QUADS):
    """Errors of the quad form and of the group form, each relative to sum |term_i|, against two exact references:
    (eq, eg) against the exact line sum -- both forms share the rounding of their common front end, above all the
    cancellation in u^2 + A2 u + Bc next to a line -- and (aq, ag) against the exact sum of the float64 quotients num / den
    of the quads, which leaves only what the two forms do differently: the accumulation."""
    t = exact_terms(u, lines)
    exact, scale = sum(t), sum(abs(x) for x in t)
    quads = [quad_terms(u, lines[k:k + 4]) for k in range(0, len(lines), 4)]
    exact_acc = sum(Fraction(float(num)) / Fraction(float(den)) for num, den in quads)
    sq, sg = Fraction(float(quad_form_sum(u, lines))), Fraction(float(group_form_sum(u, lines, group)))
    return tuple(float(abs(a - b) / scale) for a, b in ((sq, exact), (sg, exact), (sq, exact_acc), (sg, exact_acc)))
