"""instrument.Instrument without a GPU: the quadrature rules against their defining moments, the layout of the sparse map,
the refusals, the NumPy reference of the reduction (tests/obs_reference.py), and -- through the CPU oracle -- the size of
the beam effect that motivates the layer."""
import math

import numpy as np
import pytest

import obs_reference as obr

from mwr_fast_forward_operators_and_lbls_amd import _native, profiles, spectroscopy
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument, boxcar_band, gaussian_beam

FRQ = np.array([22.24, 31.4, 51.26, 58.0])
ELEV = np.array([90.0, 30.0, 10.2])
ULP = 2.0 ** -52


def per_channel():
    """Beams and bands that differ per channel: widths, an explicit double-sideband pair, a monochromatic channel."""
    sidebands = (np.array([-0.6, -0.4, 0.4, 0.6]), np.array([1.0, 3.0, 3.0, 1.0]))
    return Instrument(FRQ, ELEV, beam=[3.5, 3.5, 2.5, 2.0], band=[0.23, sidebands, None, 2.0], n_beam=3, n_band=5)


@pytest.mark.parametrize("inst", [Instrument(FRQ, ELEV, beam=3.5, band=0.23), Instrument(FRQ, ELEV, beam=3.5, n_beam=5),
                                  Instrument(FRQ, ELEV, band=2.0, n_band=2), per_channel()], ids=["both", "beam5", "band2", "mixed"])
def test_every_row_sums_to_one_and_dense_equals_the_csr(inst):
    assert inst.row_ptr[0] == 0 and inst.row_ptr[-1] == inst.col.size == inst.w.size and len(inst.row_ptr) == inst.m_out + 1
    assert inst.row_ptr.dtype == np.int32 and inst.col.dtype == np.int32 and inst.w.dtype == np.float64
    assert inst.m_in == inst.elev_q.size * inst.frq_q.size and inst.m_out == ELEV.size * FRQ.size
    assert inst.col.min() >= 0 and inst.col.max() < inst.m_in
    d = inst.dense()
    assert d.shape == (inst.m_out, inst.m_in)
    for o in range(inst.m_out):
        sl = slice(inst.row_ptr[o], inst.row_ptr[o + 1])
        assert abs(math.fsum(inst.w[sl]) - 1.0) <= 4 * ULP, (o, math.fsum(inst.w[sl]) - 1.0)
        row = np.zeros(inst.m_in)
        for c, w in zip(inst.col[sl], inst.w[sl]):
            row[c] += w
        assert np.array_equal(d[o], row)
    # the reference apply on a vector is the dense product to rounding
    x = np.random.default_rng(0).standard_normal((2, inst.m_in))
    got, scale = obr.apply_reference(inst.row_ptr, inst.col, inst.w, x)
    assert (np.abs(got - x @ d.T) <= obr.error_bar(inst.row_ptr, scale)).all()


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_gaussian_beam_rule_integrates_the_beam(n):
    fwhm = 3.5
    off, w = gaussian_beam(fwhm, n)
    ref_off, ref_w = obr.gaussian_beam_reference(fwhm, n)
    assert np.allclose(off, ref_off, rtol=1e-14, atol=0) and np.allclose(w, ref_w, rtol=1e-14, atol=0)
    sigma = fwhm / 2.3548200450309493
    assert abs(math.fsum(w) - 1.0) <= 4 * ULP
    assert abs(math.fsum(w * off)) <= 1e-15 * sigma                       # mean offset 0
    assert abs(math.fsum(w * off ** 2) - sigma ** 2) <= 1e-14 * sigma ** 2   # variance (FWHM / 2.3548)^2
    # ... and every Gaussian moment up to degree 2n - 1: E x^(2k) = sigma^2k (2k - 1)!!
    for deg in range(2 * n):
        want = 0.0 if deg % 2 else sigma ** deg * float(np.prod(np.arange(deg - 1, 0, -2)))
        assert abs(math.fsum(w * off ** deg) - want) <= 1e-12 * max(sigma ** deg, want), (n, deg)
    assert gaussian_beam(fwhm, 1)[0].tolist() == [0.0] and gaussian_beam(fwhm, 1)[1].tolist() == [1.0]


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_boxcar_rule_integrates_polynomials_to_degree_2n_minus_1(n):
    bw = 2.0
    off, w = boxcar_band(bw, n)
    if n > 1:
        ref_off, ref_w = obr.boxcar_band_reference(bw, n)
        assert np.allclose(off, ref_off, rtol=1e-14, atol=1e-17) and np.allclose(w, ref_w, rtol=1e-14, atol=0)
    assert abs(math.fsum(w) - 1.0) <= 4 * ULP and (np.abs(off) < bw / 2).all()
    for deg in range(2 * n):                                              # mean of x^deg over [-bw/2, bw/2]
        want = 0.0 if deg % 2 else (bw / 2) ** deg / (deg + 1)
        assert abs(math.fsum(w * off ** deg) - want) <= 1e-14 * (bw / 2) ** deg, (n, deg)
    deg = 2 * n                                                           # ... and no further
    assert abs(math.fsum(w * off ** deg) - (bw / 2) ** deg / (deg + 1)) > 1e-6 * (bw / 2) ** deg


def test_rows_are_angle_major_and_the_grid_is_a_tensor_grid():
    inst = Instrument(FRQ, ELEV, beam=3.5, band=0.23, n_beam=3, n_band=2)
    assert inst.elev_q.size == 9 and inst.frq_q.size == 8 and (np.diff(inst.elev_q) > 0).all() and (np.diff(inst.frq_q) > 0).all()
    nch, nf_q = FRQ.size, inst.frq_q.size
    boff, bw = obr.gaussian_beam_reference(3.5, 3)
    foff, fw = obr.boxcar_band_reference(0.23, 2)
    for a, el in enumerate(ELEV):
        for c, f in enumerate(FRQ):
            o = a * nch + c                                               # like tb[nang][nf]
            sl = slice(inst.row_ptr[o], inst.row_ptr[o + 1])
            aq, fq = np.divmod(inst.col[sl], nf_q)                        # input j = aq * nf_q + fq, like tb[nang_q][nf_q]
            assert np.allclose(np.sort(np.unique(inst.elev_q[aq])), np.sort(el + boff), rtol=1e-14)
            assert np.allclose(np.sort(np.unique(inst.frq_q[fq])), np.sort(f + foff), rtol=1e-14)
            assert sl.stop - sl.start == 6
    beams = [(boff, bw)] * nch
    bands = [(foff, fw)] * nch
    want = obr.dense_reference(FRQ, ELEV, beams, bands, inst.elev_q, inst.frq_q)
    assert np.abs(inst.dense() - want).max() <= 4 * ULP


def test_union_grid_deduplicates():
    inst = per_channel()
    # three distinct widths: centre node shared, the two outer nodes of each width distinct -> 1 + 2 * 3 per elevation
    assert inst.elev_q.size == ELEV.size * 7 and np.unique(inst.elev_q).size == inst.elev_q.size
    # 5 + 4 + 1 + 5 frequency nodes, none shared
    assert inst.frq_q.size == 15
    same = Instrument(FRQ, ELEV, beam=[3.5] * 4, band=[0.23] * 4)
    assert same.elev_q.size == ELEV.size * 3 and np.array_equal(same.dense(), Instrument(FRQ, ELEV, beam=3.5, band=0.23).dense())
    # two channels on one centre frequency share their frequency nodes; elevations whose nodes coincide share those
    twin = Instrument([31.4, 31.4], [30.0], band=0.23)
    assert twin.frq_q.size == 3 and twin.m_in == 3 and np.array_equal(twin.dense()[0], twin.dense()[1])
    shared = Instrument([31.4], [30.0, 32.0], beam=(np.array([-2.0, 0.0, 2.0]), np.array([1.0, 2.0, 1.0])))
    assert shared.elev_q.tolist() == [28.0, 30.0, 32.0, 34.0]
    # the sideband weights were normalised
    sl = slice(inst.row_ptr[1], inst.row_ptr[2])
    assert np.allclose(np.sort(np.unique(np.round(inst.w[sl] / inst.w[sl].min(), 9))), [1.0, 3.0, 4.0, 12.0])
    # a pencil-beam monochromatic instrument on ascending elevations is the identity (the grid is sorted)
    ident = Instrument(FRQ, np.sort(ELEV))
    assert np.array_equal(ident.dense(), np.eye(12)) and np.array_equal(ident.frq_q, np.sort(FRQ)) and ident.m_in == 12


def test_refusals():
    with pytest.raises(ValueError) as ei:
        Instrument(FRQ, [30.0, 4.2], beam=3.5, n_beam=5)
    text = str(ei.value)
    assert "4.2 deg" in text and "channel 0" in text and "22.24 GHz" in text and "ground pickup is not modelled" in text
    assert "largest n that fits is 4" in text
    Instrument(FRQ, [30.0, 4.2], beam=3.5, n_beam=4)                      # ... and it does
    with pytest.raises(ValueError, match=r"elevation 177 deg, channel 3 .*largest n that fits is 1"):
        Instrument(FRQ, [177.0], beam=[None, None, None, 8.0], n_beam=2)
    with pytest.raises(ValueError, match="no explicit node may lie there"):
        Instrument(FRQ, [1.0], beam=(np.array([-1.0, 1.0]), np.array([0.5, 0.5])))
    # elevations above 90 deg are passed on as they are
    over = Instrument(FRQ, [89.0], beam=3.5)
    assert over.elev_q.max() > 90.0
    # more than MWRT_MAX_ANGLES distinct elevation nodes
    assert _native.MAX_ANGLES == 64
    with pytest.raises(ValueError, match="65 distinct elevation nodes, more than MWRT_MAX_ANGLES = 64"):
        Instrument(FRQ, np.linspace(20.0, 84.0, 13), beam=3.0, n_beam=5)
    assert Instrument(FRQ, np.linspace(20.0, 84.0, 16), beam=3.0, n_beam=4).elev_q.size == 64
    with pytest.raises(ValueError, match="one entry per channel"):
        Instrument(FRQ, ELEV, beam=[3.5, 3.5])
    for bad in (dict(beam=-1.0), dict(band=float("nan")), dict(beam=3.5, n_beam=0)):
        with pytest.raises(ValueError):
            Instrument(FRQ, ELEV, **bad)


def test_onedvar_refuses_a_mismatched_instrument():
    torch = pytest.importorskip("torch")
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    inst = Instrument(FRQ, ELEV, beam=3.5)
    nlev, m = 4, inst.m_out
    args = dict(sa=torch.eye(2 * nlev, dtype=torch.float64), se=torch.ones(m, dtype=torch.float64),
                xa=torch.zeros((2, nlev), dtype=torch.float64))
    ov = retrieval.OneDVar("R24", FRQ, ELEV, args["sa"], args["se"], xa=args["xa"], instrument=inst)
    assert ov.m == inst.m_out == 12
    for frq, elev in ((FRQ[:3], ELEV), (FRQ, ELEV[::-1]), (FRQ + 0.01, ELEV)):
        with pytest.raises(ValueError, match="must equal the instrument's channel centres and elevations"):
            retrieval.OneDVar("R24", frq, elev, args["sa"], args["se"], xa=args["xa"], instrument=inst)


def test_reference_apply_confines_nan_to_the_rows_that_reference_it():
    inst = Instrument(FRQ, ELEV, beam=3.5, band=0.23, n_band=2)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, inst.m_in, 5)) + 200.0
    clean, _ = obr.apply_reference(inst.row_ptr, inst.col, inst.w, x)
    j = int(inst.col[inst.row_ptr[5]])                                    # a node of row 5
    x[1, j, 2] = np.nan
    got, _ = obr.apply_reference(inst.row_ptr, inst.col, inst.w, x)
    hit = np.array([j in inst.col[inst.row_ptr[o]:inst.row_ptr[o + 1]] for o in range(inst.m_out)])
    assert hit[5] and 1 <= hit.sum() < inst.m_out
    want_nan = np.zeros(got.shape, dtype=bool)
    want_nan[1, hit, 2] = True
    assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(got[~want_nan], clean[~want_nan])
    # ... which the dense product does not: 0 * NaN reaches every row
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.einsum("oj,pjl->pol", inst.dense(), x)[1, :, 2]).all()
    # a NaN elevation is one node of the grid and reaches that elevation's channels alone
    nan_el = Instrument(FRQ, [90.0, float("nan"), 30.0], beam=3.5)
    assert nan_el.elev_q.size == 7 and np.isnan(nan_el.elev_q[-1]) and np.isnan(nan_el.elev_q).sum() == 1
    tb = np.where(np.isnan(nan_el.elev_q)[:, None], np.nan, 250.0) * np.ones((1, 7, 4))
    out, _ = obr.apply_reference(nan_el.row_ptr, nan_el.col, nan_el.w, tb.reshape(1, -1))
    assert np.array_equal(np.isnan(out.reshape(3, 4)), np.array([[False] * 4, [True] * 4, [False] * 4]))


def test_the_beam_effect_that_motivates_the_layer():
    """R98, synthetic_profiles(2, nlev=60)[0], a 3.5 deg beam, through the CPU oracle: channel minus centre TB at 31.4 GHz
    is above 1 K at 4.2 deg (5.7 K) and below 0.05 K at zenith (0.007 K); 3 and 5 beam nodes agree within 0.2 K at 5.4 deg
    (0.13 K)."""
    from oracle import lbl_oracle
    pr = profiles.synthetic_profiles(2, nlev=60)
    tables = spectroscopy.get_model("R98")
    frq = np.array([22.24, 31.4, 51.26])

    def channel_tb(inst):
        r = lbl_oracle.tb_cloud_rte(tables, pr["z"][0], pr["p"][0], pr["t"][0], pr["rh"][0], inst.frq_q, inst.elev_q)
        out, _ = obr.apply_reference(inst.row_ptr, inst.col, inst.w, r["tbtotal"].reshape(1, -1))
        return out.reshape(inst.elev.size, frq.size)

    elev = [90.0, 5.4, 4.2]
    centre = channel_tb(Instrument(frq, elev))
    beam3 = channel_tb(Instrument(frq, elev, beam=3.5, n_beam=3))
    d = beam3 - centre
    print("channel minus centre TB [K], rows 90 / 5.4 / 4.2 deg, columns 22.24 / 31.4 / 51.26 GHz:\n", d)
    assert d[2, 1] > 1.0 and abs(d[0, 1]) < 0.05
    beam5 = channel_tb(Instrument(frq, [5.4], beam=3.5, n_beam=5))
    print("5 minus 3 beam nodes at 5.4 deg [K]:", beam5[0] - beam3[1])
    assert np.abs(beam5[0] - beam3[1]).max() < 0.2
