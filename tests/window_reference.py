"""The window plan of the fine-grid absorption kernel (k_absorb_win), restated without library code: NumPy, Python floats
where the planner decides in doubles (so a decision can be compared bit for bit), ``np.longdouble`` where an error of
1e-13 or more is measured, mpmath where a figure is confirmed (``confirm_with_mpmath``).

What the planner (csrc/mwrt_plan.cpp: build_windows, window_far_sets, window_nodes, chunk_masks) decides from the
frequencies and the line centres alone, and where each rule comes from:

* base windows -- 8 chunks of 16 frequencies; one workgroup sums the window-far lines once at Chebyshev nodes of
  [first, last frequency] and interpolates them to the 128 targets.  A list is eligible with >= 128 increasing
  frequencies, every base window <= 6 GHz wide and no one-frequency last window (no span to put nodes on).
* far sets -- a line's term is analytic in f with poles at c +- i w.  Polynomial interpolation on Chebyshev nodes of
  an interval of half-span h converges like rho^-n with rho = d/h + sqrt((d/h)^2 - 1) for a pole at distance d from
  the interval's middle, i.e. it is the RATIO of the distance to the half-span that sets the error, not the distance:
    O2,  16 nodes: margin beyond the window >= max(4 GHz, 1.6 h): d/h >= 2.6, rho >= 5, 5^-16 = 6.6e-12 times the
                   growth of the term towards the pole -- measured 3e-10 .. 4e-10 of the line's own term at ratio 2.6;
    H2O,  8 nodes: margin >= max(30 GHz, 11.8 h): d/h >= 12.8, rho >= 25.6, 25.6^-8 = 5.4e-12.
  The floor (4 / 30 GHz) is the ratio at the 5-GHz span the kernel was sized on (h = 2.5); the ratio term keeps it for
  the wider (<= 6 GHz, merged: <= 12 GHz) windows.
* speed-dependent reach -- ABH2O_SD replaces the resonant Lorentzian by the speed-dependent shape inside 10
  half-widths, a per-level switch: not analytic, so such a line joins a far set only where 10 half-widths (bounded over
  any atmosphere: dry air <= 1100 hPa, vapour <= 150 hPa, (Tref / T)^x <= 2^x) plus 1 GHz for the pressure shift
  cannot reach the window; the kernel re-checks per level with the actual width and takes the line back.
* cutoff classes -- each Lorentz term is cut at |f -+ c| = 750 GHz.  A far line's sum is smooth across the window only
  if each term is in or out for the whole window at every level: a 5-GHz guard (pressure shifts < 1 GHz) either side
  of 750.  Both in: ``h2o_far_both``; resonant in, negative-frequency term out: ``h2o_far_res``; else: the chunk loops.
* merge -- two neighbouring base windows (the first one full) share one node phase when the merged window has EVERY
  O2 line far and its H2O far set is what the two had in common (nothing leaves the far set by merging).
* sdint -- the speed-dependent shape MINUS its Lorentzian is evaluated at slots 0, 2, .., 14, 15 of a full chunk of
  increasing frequencies and interpolated (degree 8) to the odd slots where the chunk is >= 3 GHz (the difference's
  own scale: a few half-widths at the levels where it matters) and >= 5 chunk spans (ratio 11: rho ~ 22, 22^-9 = 8e-13)
  from the centre -- and only where the chunk's own slots interpolate stably: the sum of a target's |weights| (10.3 on an
  evenly spaced chunk) multiplies every rounding error of the nine samples; near-coincident frequencies next to a gap
  reach 1e4, and such a chunk is sampled in full (its weights are left zero).
* chunk masks -- the every-line classification per 16-frequency chunk (mwrt_plan.h LineMasks): direct-form distance
  0.2 + 0.05 GHz for O2, 5 GHz for H2O, the 750 + 5 GHz cutoff classes, the very-far Taylor sets (poles in f^2 at
  >= 1 / 0.016 half ranges, at least 4 lines, at least 7 frequencies).
"""
import numpy as np

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")

WIN_CHUNKS, WIN_CHUNKS_MAX, WIN_NFC = 8, 16, 16
WIN_NODES, WIN_NODES_H = 16, 8
PER = WIN_CHUNKS * WIN_NFC
O2_MARGIN_GHZ, O2_RATIO = 4.0, 1.6
H2O_MARGIN_GHZ, H2O_RATIO = 30.0, 11.8
MAX_SPAN_GHZ = 6.0
CUTOFF_GHZ, GUARD_GHZ = 750.0, 5.0
SD_NODE_SLOTS = (0, 2, 4, 6, 8, 10, 12, 14, 15)
SD_TARGET_SLOTS = (1, 3, 5, 7, 9, 11, 13)
SD_MIN_GHZ, SD_MIN_SPANS = 3.0, 5.0
SD_LEBESGUE_MAX = 100.0                      # nine weights rounded to doubles still sum to 1 within 9 x 100 x 2^-53 = 1e-13
FAR_O2_GHZ = 0.2 + 0.05                      # direct-form distance + shift allowance
FAR_H2O_GHZ = 5.0
VF_RATIO_MAX, VF_MIN_FREQS, VF_MIN_LINES = 0.016, 7, 4


# ---------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------
def eligible(frq):
    frq = [float(x) for x in frq]
    if len(frq) < PER or any(not b > a for a, b in zip(frq, frq[1:])):
        return False
    for b in range(0, len(frq), PER):
        e = min(len(frq), b + PER) - 1
        if e == b or frq[e] - frq[b] > MAX_SPAN_GHZ:
            return False
    return True


def sd_halfwidth_bound(m, k):
    """largest half-width [GHz] of H2O line k in any atmosphere: width0 = w0 pda ti^x + w0s pvap ti^xs at pda = 1100 hPa,
    pvap = 150 hPa, ti = Tref / T = 2 (T = 148 .. 150 K)"""
    L = m.h2o
    return (float(L["w0"][k]) * 1100.0 * 2.0 ** max(float(L["x"][k]), 0.0)
            + float(L["w0s"][k]) * 150.0 * 2.0 ** max(float(L["xs"][k]), 0.0))


def far_sets(m, flo, fhi):
    """-> (o2_far, h2o_far_both, h2o_far_res) of the window [flo, fhi], as bit sets over the line tables"""
    flo, fhi = float(flo), float(fhi)
    half = 0.5 * (fhi - flo)
    mo, mh = max(O2_MARGIN_GHZ, O2_RATIO * half), max(H2O_MARGIN_GHZ, H2O_RATIO * half)
    o2 = both = res = 0
    for k, c in enumerate(float(x) for x in m.o2["f"]):
        if c < flo - mo or c > fhi + mo:
            o2 |= 1 << k
    for k, c in enumerate(float(x) for x in m.h2o["fl"]):
        if not (c < flo - mh or c > fhi + mh):
            continue
        if float(m.h2o["w2"][k]) > 0.0 and not 10.0 * sd_halfwidth_bound(m, k) < min(abs(c - flo), abs(c - fhi)) - 1.0:
            continue
        inside = CUTOFF_GHZ - GUARD_GHZ
        d1_in = abs(flo - c) < inside and abs(fhi - c) < inside
        if d1_in and fhi + c < inside:
            both |= 1 << k
        elif d1_in and flo + c >= CUTOFF_GHZ + GUARD_GHZ:
            res |= 1 << k
    return o2, both, res


def bounds(span, nf):
    """(first chunk, chunks) -> index of the first and the last frequency"""
    c0, nch = span
    return c0 * WIN_NFC, min(nf, (c0 + nch) * WIN_NFC) - 1


def base_spans(nf):
    nchunks = -(-nf // WIN_NFC)
    return [(w * WIN_CHUNKS, min(WIN_CHUNKS, nchunks - w * WIN_CHUNKS)) for w in range(-(-nf // PER))]


def may_merge(m, frq, a, b):
    """the merge rule for neighbouring spans a, b"""
    nf = len(frq)
    if a[1] != WIN_CHUNKS or a[1] + b[1] > WIN_CHUNKS_MAX:
        return False
    ends = lambda s: (frq[bounds(s, nf)[0]], frq[bounds(s, nf)[1]])
    om, bm, rm = far_sets(m, *ends((a[0], a[1] + b[1])))
    _, b0, r0 = far_sets(m, *ends(a))
    _, b1, r1 = far_sets(m, *ends(b))
    return om == (1 << m.n_o2) - 1 and (bm | rm) == ((b0 | r0) & (b1 | r1))


def spans_of(m, frq):
    """the windows in grid order, merged left to right (a merged window is not merged again)"""
    spans = base_spans(len(frq))
    i = 0
    while i + 1 < len(spans):
        if may_merge(m, frq, spans[i], spans[i + 1]):
            spans[i:i + 2] = [(spans[i][0], spans[i][1] + spans[i + 1][1])]
        i += 1
    return spans


def chunk_masks(m, frq):
    """the width-16 LineMasks of every chunk, as dicts of the fields the dump prints"""
    frq = [float(x) for x in frq]
    nf = len(frq)
    out = []
    for j0 in range(0, nf, WIN_NFC):
        f = frq[j0:j0 + WIN_NFC]
        u = [x * x for x in f]
        u0, h = 0.5 * (min(u) + max(u)), max(0.5 * (max(u) - min(u)), 1.0)

        def very_far(c):
            lo, hi = max(c - 2.0, 0.0), c + 2.0
            plo, phi = lo * lo - 100.0, hi * hi
            dist = plo - u0 if u0 < plo else (u0 - phi if u0 > phi else 0.0)
            return h <= VF_RATIO_MAX * dist
        vfar_ok = len(f) >= VF_MIN_FREQS
        d = dict(o2_far=0, o2_vfar=0, h2o_far=0, h2o_vfar=0, h2o_none=0, h2o_res=0, h2o_sd=0, h2o_sdfar=0, h2o_sdint=0,
                 vf_u0=u0, vf_h=h)
        for k, c in enumerate(float(x) for x in m.o2["f"]):
            if min(abs(x - c) for x in f) >= FAR_O2_GHZ:
                d["o2_far"] |= 1 << k
            if vfar_ok and very_far(c):
                d["o2_vfar"] |= 1 << k
        if bin(d["o2_vfar"]).count("1") < VF_MIN_LINES:
            d["o2_vfar"] = 0
        increasing = sd_half_ok(f)
        for k, c in enumerate(float(x) for x in m.h2o["fl"]):
            dmin, smin = min(abs(x - c) for x in f), min(abs(x + c) for x in f)
            out_of_cutoff = CUTOFF_GHZ + FAR_H2O_GHZ
            if dmin >= FAR_H2O_GHZ:
                d["h2o_far"] |= 1 << k
            if vfar_ok and very_far(c):
                d["h2o_vfar"] |= 1 << k
            if dmin >= out_of_cutoff and smin >= out_of_cutoff:
                d["h2o_none"] |= 1 << k
            if smin >= out_of_cutoff:
                d["h2o_res"] |= 1 << k
            if float(m.h2o["w2"][k]) > 0.0:
                d["h2o_sd"] |= 1 << k
                if 10.0 * sd_halfwidth_bound(m, k) < dmin - 1.0:
                    d["h2o_sdfar"] |= 1 << k
                if increasing and dmin >= SD_MIN_GHZ and dmin >= SD_MIN_SPANS * (f[-1] - f[0]):
                    d["h2o_sdint"] |= 1 << k
        if bin(d["h2o_vfar"]).count("1") < VF_MIN_LINES:
            d["h2o_vfar"] = 0
        out.append(d)
    return out


def sd_half_ok(f):
    """may the chunk be half-sampled: 16 increasing frequencies, and no odd slot whose nine weights sum to more than
    SD_LEBESGUE_MAX in absolute value"""
    if len(f) != WIN_NFC or any(not b > a for a, b in zip(f, f[1:])):
        return False
    f = np.asarray(f, dtype=np.float64)
    nodes = f[list(SD_NODE_SLOTS)]
    return all(np.abs(lagrange_weights(nodes, x)).sum() <= SD_LEBESGUE_MAX for x in f[list(SD_TARGET_SLOTS)])


def chebyshev_nodes(flo, fhi, n):
    """the n Chebyshev nodes of [flo, fhi] in extended precision (first node nearest fhi)"""
    flo, fhi = LD(flo), LD(fhi)
    k = np.arange(n, dtype=LD)
    return 0.5 * (flo + fhi) + 0.5 * (fhi - flo) * np.cos(PI * (2 * k + 1) / (2 * n))


def lagrange_weights(nodes, x):
    """w[m] with p(x) = sum_m w[m] p(nodes[m]) for every polynomial p of degree < len(nodes), in extended precision"""
    nodes, x = np.asarray(nodes, dtype=LD), LD(x)
    w = np.ones(len(nodes), dtype=LD)
    for m in range(len(nodes)):
        for q in range(len(nodes)):
            if q != m:
                w[m] *= (x - nodes[q]) / (nodes[m] - nodes[q])
    return w


# ---------------------------------------------------------------------------------------------------------------------
# a dumped plan (tests/plan_dump.cpp `windows`) as arrays
# ---------------------------------------------------------------------------------------------------------------------
def plan_arrays(dump, frq):
    """the JSON answer -> the same with the weight blocks as arrays: window["lag"] [chunk][node][target],
    window["lag_h"] likewise, plan["lag_sd"] [chunk][target][node], plan["frq"]"""
    plan = dict(dump, frq=np.asarray(frq, dtype=np.float64), windows=[])
    for w in dump["windows"]:
        w = dict(w)
        w["lag"] = np.array(w["lag"], dtype=np.float64).reshape(w["nchunks"], WIN_NODES, WIN_NFC)
        w["lag_h"] = np.array(w["lag_h"], dtype=np.float64).reshape(w["nchunks"], WIN_NODES_H, WIN_NFC)
        plan["windows"].append(w)
    plan["lag_sd"] = np.array(dump["lag_sd"], dtype=np.float64).reshape(-1, len(SD_TARGET_SLOTS), len(SD_NODE_SLOTS))
    return plan


def window_targets(plan, w):
    """indices into plan["frq"] of the window's targets (the real ones: no padding)"""
    nf = len(plan["frq"])
    return np.arange(w["first_chunk"] * WIN_NFC, min(nf, (w["first_chunk"] + w["nchunks"]) * WIN_NFC))


def interpolate(block, values, ntargets):
    """node values [..., node] through a [chunk][node][target] block -> [..., target] for the first `ntargets` targets"""
    nch, nn, _ = block.shape
    flat = np.transpose(block.astype(LD), (1, 0, 2)).reshape(nn, nch * WIN_NFC)[:, :ntargets]
    return values @ flat


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's line terms (oracle/lbl_oracle.py o2_absorption / h2o_absorption, statement for statement) in extended
# precision, per line set: [level][frequency]
# ---------------------------------------------------------------------------------------------------------------------
def _bits(mask):
    return [k for k in range(mask.bit_length()) if (mask >> k) & 1]


def level_state(p, t, rh):
    """what both routines start from: e [hPa] (Goff-Gratch, as RTEquation.vapor), then pyrtlib's unit round trips"""
    p, t, rh = (np.asarray(x, dtype=LD) for x in (p, t, rh))
    y = LD(373.16) / t
    es = (LD(-7.90298) * (y - 1) + LD(5.02808) * np.log10(y) - LD(1.3816e-07) * (10 ** (LD(11.344) * (1 - 1 / y)) - 1)
          + LD(0.0081328) * (10 ** (LD(-3.49149) * (y - 1)) - 1) + np.log10(LD(1013.246)))
    e = rh * 10 ** es
    ekpa = e / 10
    return dict(t=t, ekpa=ekpa, pdrykpa=p / 10 - ekpa)


def o2_scale(m, st):
    """adry = o2_scale * (line sum + non-resonant term) + N2"""
    vx = 300 / st["t"]
    temp = 300 / vx
    pres = (st["pdrykpa"] + st["ekpa"]) * 10
    vapden = st["ekpa"] * 10 / (LD(0.01 * 8.314510) / LD(18.01528) * temp)
    presda = pres - vapden * temp / LD(m.o2_pvap_div)
    return LD(m.o2_coef) * presda * (300 / temp) ** 3


def o2_line_sum(m, st, f, lines):
    f = np.asarray(f, dtype=LD)[None, :]
    rvap = LD(0.01 * 8.314510) / LD(18.01528)
    temp = 300 / (300 / st["t"])
    pres = (st["pdrykpa"] + st["ekpa"]) * 10
    vapden = st["ekpa"] * 10 / (rvap * temp)
    th = 300 / temp
    th1 = th - 1
    b = th ** LD(m.o2_x)
    preswv = vapden * temp / LD(m.o2_pvap_div)
    presda = pres - preswv
    den = LD(0.001) * (presda * b + LD(m.o2_wv_factor) * preswv * th)
    dens = LD(0.001) * (presda + LD(m.o2_wv_factor) * preswv) * th
    pe2 = den * den
    L = {k: v.astype(LD) for k, v in m.o2.items()}
    col = lambda x: x[:, None]
    out = np.zeros((len(st["t"]), f.shape[1]), dtype=LD)
    for k in lines:
        strr = L["s300"][k] * np.exp(-L["be"][k] * th1)
        if m.o2_mix_mode == 0:
            df = L["w300"][k] * (dens if (k == 0 and m.o2_line1_dens) else den)
            y = LD(0.001) * pres * b * (L["y0"][k] + L["y1"][k] * th1)
            d1, d2 = f - L["f"][k], f + L["f"][k]
            sf1 = (col(df) + d1 * col(y)) / (d1 ** 2 + col(df * df))
            sf2 = (col(df) - d2 * col(y)) / (d2 ** 2 + col(df * df))
        else:
            y = den * (L["y0"][k] + L["y1"][k] * th1)
            dnu = pe2 * (L["dnu0"][k] + L["dnu1"][k] * th1)
            gfac = 1 + pe2 * (L["g0"][k] + L["g1"][k] * th1)
            df = L["w300"][k] * den
            d1, d2 = f - L["f"][k] - col(dnu), f + L["f"][k] + col(dnu)
            sf1 = (col(df * gfac) + d1 * col(y)) / (d1 * d1 + col(df * df))
            sf2 = (col(df * gfac) - d2 * col(y)) / (d2 * d2 + col(df * df))
        out += col(strr) * (sf1 + sf2) * (f / L["f"][k]) ** 2
    return out


def h2o_state(m, st):
    rvap = LD(0.01 * 8.314510) / LD(18.01528)
    t = 300 / (300 / st["t"])
    rho = st["ekpa"] * 10 / (rvap * t)
    pvap = rho * t / LD(m.h2o_pvap_div)
    pda = (st["pdrykpa"] + st["ekpa"]) * 10 - pvap
    ti = LD(m.h2o_reftline) / t
    return dict(t=t, rho=rho, pvap=pvap, pda=pda, ti=ti, tiln=np.log(ti), scale=LD(3.183e-05) * LD(m.h2o_den_coef) * rho)


def h2o_line(m, hs, k):
    """per level: width0, width2, delta2, shift, strength of line k"""
    L = {key: LD(v[k]) for key, v in m.h2o.items()}
    ti, tiln, pda, pvap = hs["ti"], hs["tiln"], hs["pda"], hs["pvap"]
    width0 = L["w0"] * pda * ti ** L["x"] + L["w0s"] * pvap * ti ** L["xs"]
    width2 = L["w2"] * pda * ti ** L["xw2"] + L["w2s"] * pvap * ti ** L["xw2s"] if L["w2"] > 0 else np.zeros_like(ti)
    delta2 = L["d2"] * pda + L["d2s"] * pvap
    if m.h2o_shift_mode == 0:
        shift = np.zeros_like(ti)
    else:
        shift = (L["sh"] * pda * (1 - L["aair"] * tiln) * ti ** L["xh"] + L["shs"] * pvap * (1 - L["aself"] * tiln) * ti ** L["xhs"])
    s = L["s1"] * ti ** LD(2.5) * np.exp(L["b2"] * (1 - ti))
    return dict(fl=L["fl"], width0=width0, width2=width2, delta2=delta2, shift=shift, s=s)


def h2o_line_sum(m, hs, f, both, res):
    """the cut-off Lorentzians of the lines in `both` (two terms) and `res` (resonant term only), as the far sets promise
    them: no speed-dependent shape, the cutoff state uniform"""
    f = np.asarray(f, dtype=LD)[None, :]
    out = np.zeros((len(hs["t"]), f.shape[1]), dtype=LD)
    col = lambda x: x[:, None]
    for k in _bits(both | res):
        q = h2o_line(m, hs, k)
        wsq = q["width0"] ** 2
        base = q["width0"] / (562500 + wsq)
        d1 = f - q["fl"] - col(q["shift"])
        term = col(q["width0"]) / (d1 ** 2 + col(wsq)) - col(base)
        if (both >> k) & 1:
            d2 = f + q["fl"] + col(q["shift"])
            term = term + col(q["width0"]) / (d2 ** 2 + col(wsq)) - col(base)
        out += col(q["s"]) * term * (f / q["fl"]) ** 2
    return out


def dcerror(z_re, z_im):
    """Rosenkranz DCERROR (Hui, Armstrong & Wray 1978), upper half plane, in extended precision"""
    a = [122.607931777104326, 214.382388694706425, 181.928533092181549, 93.155580458138441, 30.180142196210589,
         5.912626209773153, 0.564189583562615]
    b = [122.607931773875350, 352.730625110963558, 457.334478783897737, 348.703917719495792, 170.354001821091472,
         53.992906912940207, 10.479857114260399]
    zh = (np.abs(z_im) - 1j * z_re).astype(np.clongdouble)
    asum = zh * 0 + LD(a[6])
    for c in a[5::-1]:
        asum = asum * zh + LD(c)
    bsum = zh + LD(b[6])
    for c in b[5::-1]:
        bsum = bsum * zh + LD(c)
    return asum / bsum


def sd_difference(m, hs, k, f):
    """(speed-dependent resonant shape - the Lorentzian it replaces) [level][frequency], and where the oracle applies it"""
    f = np.asarray(f, dtype=LD)[None, :]
    q = h2o_line(m, hs, k)
    col = lambda x: x[:, None]
    d1 = f - q["fl"] - col(q["shift"])
    inner = (col(q["width2"]) > 0) & (np.abs(d1) < 10 * col(q["width0"]))
    w2 = np.where(q["width2"] > 0, q["width2"], LD(1))                 # (levels without a shape: never inner)
    den = (col(w2) - 1j * col(q["delta2"])).astype(np.clongdouble)
    xc = ((col(q["width0"]) - LD(1.5) * col(w2)) + 1j * (d1 + LD(1.5) * col(q["delta2"]))) / den
    xrt = np.sqrt(xc)
    pxw = LD(1.77245385090551603) * xrt * dcerror(-xrt.imag, xrt.real)
    sd = (2 * (1 - pxw) / den).real
    return sd - col(q["width0"]) / (d1 ** 2 + col(q["width0"] ** 2)), inner, q


# ---------------------------------------------------------------------------------------------------------------------
# what the plan costs in accuracy
# ---------------------------------------------------------------------------------------------------------------------
def plan_truncation(plan, m, profile, levels=None):
    """Largest error the PLAN alone leaves in the absorption of `profile` (dict of p, t, rh [nlev]) at `levels`, before any
    rounding on the device: the oracle's line terms of each window's far sets at the dumped nodes, interpolated with
    the dumped weights, against the same terms at the targets.  Relative to lbl_oracle's total dry / wet absorption
    at that level and frequency.  -> dict(dry, wet, sd): the maxima over windows, levels and frequencies; ``sd`` is the
    half-sampled speed-dependent shape (lag_sd), relative to the wet absorption."""
    from oracle import lbl_oracle as lo
    frq = plan["frq"]
    p, t, rh = (np.asarray(profile[k], dtype=np.float64) for k in ("p", "t", "rh"))
    levels = np.arange(len(p)) if levels is None else np.asarray(levels)
    aw, ad = lo.absorption_profile(m, p[levels], t[levels], rh[levels], frq)       # [nf][level]
    st = level_state(p[levels], t[levels], rh[levels])
    hs = h2o_state(m, st)
    out = dict(dry=0.0, wet=0.0, sd=0.0)
    for w in plan["windows"]:
        idx = window_targets(plan, w)
        lines = _bits(w["o2_far"])
        if lines:
            nodes = o2_line_sum(m, st, w["fnode"], lines)
            err = interpolate(w["lag"], nodes, len(idx)) - o2_line_sum(m, st, frq[idx], lines)
            out["dry"] = max(out["dry"], float(np.max(np.abs(err * o2_scale(m, st)[:, None]) / ad[idx].T)))
        if w["h2o_far_both"] | w["h2o_far_res"]:
            nodes = h2o_line_sum(m, hs, w["fnode_h"], w["h2o_far_both"], w["h2o_far_res"])
            err = interpolate(w["lag_h"], nodes, len(idx)) - h2o_line_sum(m, hs, frq[idx], w["h2o_far_both"], w["h2o_far_res"])
            out["wet"] = max(out["wet"], float(np.max(np.abs(err * hs["scale"][:, None]) / aw[idx].T)))
    for ch, mask in enumerate(plan["masks"]):
        for k in _bits(mask["h2o_sdint"]):
            f = frq[ch * WIN_NFC:(ch + 1) * WIN_NFC]
            diff, inner, q = sd_difference(m, hs, k, f)
            tgt = list(SD_TARGET_SLOTS)
            err = (diff[:, list(SD_NODE_SLOTS)] @ plan["lag_sd"][ch].astype(LD).T - diff[:, tgt]) * inner[:, tgt]
            err = err * (q["s"] * hs["scale"])[:, None] * (np.asarray(f[tgt], dtype=LD)[None, :] / q["fl"]) ** 2
            out["sd"] = max(out["sd"], float(np.max(np.abs(err) / aw[ch * WIN_NFC:(ch + 1) * WIN_NFC][tgt].T)))
    return out


def sd_reach(m, p, t, rh, k):
    """10 actual half-widths [GHz] of H2O line k per level, and its shifted centre: what the kernel's per-level vote
    compares with the distance to the window (the oracle's width formula)"""
    hs = h2o_state(m, level_state(p, t, rh))
    q = h2o_line(m, hs, k)
    return np.asarray(10 * q["width0"], dtype=np.float64), np.asarray(q["fl"] + q["shift"], dtype=np.float64)


def confirm_with_mpmath(m, profile, level, w, idx, frq, species, digits=30):
    """One window's truncation at one level with every step in mpmath at `digits` digits (level state from the
    extended-precision one: its 19 digits are inputs here, not the quantity confirmed) -> the error relative to the far
    lines' own sum, next to the same figure from the extended-precision path"""
    import mpmath as mp
    mp.mp.dps = digits
    st = level_state(*(np.asarray(profile[k])[[level]] for k in ("p", "t", "rh")))
    hs = h2o_state(m, st)
    f_nodes = w["fnode"] if species == "o2" else w["fnode_h"]
    block = w["lag"] if species == "o2" else w["lag_h"]
    if species == "o2":
        term_ld = lambda f: o2_line_sum(m, st, f, _bits(w["o2_far"]))[0]
    else:
        term_ld = lambda f: h2o_line_sum(m, hs, f, w["h2o_far_both"], w["h2o_far_res"])[0]
    got_ld = interpolate(block, term_ld(f_nodes)[None, :], len(idx))[0]
    want_ld = term_ld(frq[idx])
    ld = float(np.max(np.abs(got_ld - want_ld) / np.abs(want_ld)))

    # the same line terms as rational functions of f, coefficients from the level state, evaluated in mpmath
    mpf = lambda x: mp.mpf(repr(float(x))) + mp.mpf(repr(float(LD(x) - LD(float(x)))))

    def term_mp(f):
        f = mpf(f)
        tot = mp.mpf(0)
        if species == "o2":
            for k in _bits(w["o2_far"]):
                unit = o2_line_coefficients(m, st, k)
                d1, d2 = f - unit["c"], f + unit["c"]
                tot += unit["s"] * ((unit["wg"] + d1 * unit["y"]) / (d1 * d1 + unit["w"] ** 2)
                                    + (unit["wg"] - d2 * unit["y"]) / (d2 * d2 + unit["w"] ** 2)) * (f / unit["f"]) ** 2
        else:
            for k in _bits(w["h2o_far_both"] | w["h2o_far_res"]):
                q = h2o_line(m, hs, k)
                w0, c, s, fl = mpf(q["width0"][0]), mpf(q["fl"] + q["shift"][0]), mpf(q["s"][0]), mpf(q["fl"])
                base = w0 / (562500 + w0 * w0)
                term = w0 / ((f - c) ** 2 + w0 * w0) - base
                if (w["h2o_far_both"] >> k) & 1:
                    term += w0 / ((f + c) ** 2 + w0 * w0) - base
                tot += s * term * (f / fl) ** 2
        return tot
    nodes_mp = [term_mp(x) for x in f_nodes]
    flat = np.transpose(block, (1, 0, 2)).reshape(len(f_nodes), -1)[:, :len(idx)]
    worst = mp.mpf(0)
    for j, i in enumerate(idx):
        want = term_mp(frq[i])
        got = mp.fsum(mpf(flat[n, j]) * nodes_mp[n] for n in range(len(f_nodes)))
        worst = max(worst, abs(got - want) / abs(want))
    return float(worst), ld


def o2_line_coefficients(m, st, k):
    """line k's term at the single level of `st` as mpmath numbers: s [(wg + d1 y) / (d1^2 + w^2) + (wg - d2 y) / (d2^2 + w^2)] (f / f0)^2"""
    import mpmath as mp
    mpf = lambda x: mp.mpf(repr(float(x))) + mp.mpf(repr(float(LD(x) - LD(float(x)))))
    # probe the extended-precision routine for the coefficients: evaluate its pieces through the same statements
    rvap = LD(0.01 * 8.314510) / LD(18.01528)
    temp = 300 / (300 / st["t"])
    pres = (st["pdrykpa"] + st["ekpa"]) * 10
    vapden = st["ekpa"] * 10 / (rvap * temp)
    th = 300 / temp
    th1 = th - 1
    b = th ** LD(m.o2_x)
    preswv = vapden * temp / LD(m.o2_pvap_div)
    presda = pres - preswv
    den = LD(0.001) * (presda * b + LD(m.o2_wv_factor) * preswv * th)
    dens = LD(0.001) * (presda + LD(m.o2_wv_factor) * preswv) * th
    L = {key: LD(v[k]) for key, v in m.o2.items()}
    s = L["s300"] * np.exp(-L["be"] * th1)
    if m.o2_mix_mode == 0:
        w = L["w300"] * (dens if (k == 0 and m.o2_line1_dens) else den)
        y = LD(0.001) * pres * b * (L["y0"] + L["y1"] * th1)
        wg, c = w, L["f"] + 0 * w
    else:
        y = den * (L["y0"] + L["y1"] * th1)
        c = L["f"] + den * den * (L["dnu0"] + L["dnu1"] * th1)
        w = L["w300"] * den
        wg = w * (1 + den * den * (L["g0"] + L["g1"] * th1))
    return dict(s=mpf(s[0]), w=mpf(w[0]), wg=mpf(wg[0]), y=mpf(y[0]), c=mpf(c[0]), f=mpf(L["f"]))
