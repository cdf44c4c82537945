"""retrieval.OneDVar.characterise_nform without a GPU: the seams to the native library are replaced as in
tests/test_retrieval_nform_cpu.py, the two new ones by the NumPy reference of tests/nform_char_reference.py.  What is
checked is the module's own work: ``characterise_nform`` gives what ``characterise`` of a ``form="m"`` twin gives on the same
case, to 2 * nform_reference.TOL in the units of ``char_errors`` (two forms of one step differ by the rounding of two
factorisations) -- plain, with a basis, with an instrument, with ``se=`` in both per-profile shapes (the gain un-whitened)
and with a missing observation; with ``form="m"`` nothing reaches the new seams; ``gain=False`` skips the gain seam; ``rows=``
is validated and passed through; a case of m = 154 observations runs."""
import numpy as np
import pytest

import nform_char_reference as ncr
import nform_reference as nfr

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd import retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402
from test_retrieval_basis_cpu import N, R, eofs  # noqa: E402
from test_retrieval_instrument_cpu import ELEV, FRQ, M, NLEV, NPROF, make, setup  # noqa: E402
from test_retrieval_nform_cpu import NfStandins, pair  # noqa: E402
from test_retrieval_se_cpu import observations, se_batch  # noqa: E402

BAR = 2 * nfr.TOL
FIELDS = ("gain", "avk", "avk_diag", "dfs_block", "noise_var", "smooth_var", "post_cov")


class NfCharStandins(NfStandins):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.nf_chars, self.nf_gains = [], []
        for name in ("oe_nform_char", "oe_nform_gain"):
            monkeypatch.setattr(retrieval, "_native_" + name, getattr(self, name))

    def oe_nform_char(self, sa_inv, lin, nblk, out, rows, stream):
        self.order.append("nform_char")
        ref = ncr.char_linearisation(lin["h"].numpy(), lin["lin_status"].numpy(), sa_inv.numpy(), nblk, rows)
        self.nf_chars.append(dict(asked=sorted(out), rows=rows, nblk=nblk, ref=ref))
        for key, v in out.items():
            v[...] = torch.as_tensor(ref["post_cov_full" if key == "post_cov" else key]).reshape(v.shape)

    def oe_nform_gain(self, k_blocks, se, keep, post_cov, status, stream):
        self.order.append("nform_gain")
        nprof, m = keep.shape
        self.nf_gains.append(dict(k=list(k_blocks), se=se, post_cov=post_cov))
        return torch.as_tensor(ncr.gain_rows([k.numpy().reshape(nprof, m, -1) for k in k_blocks], se.numpy(), keep.numpy(),
                                             post_cov.numpy(), status.numpy()))


def char_errors(ch_n, ch_m, bounds, sa):
    """``char_errors`` of two Characterisations, the m-form twin as the reference with the bound matrices |S^| |H| the char
    seam's reference returned."""
    got = {key: getattr(ch_n, key).numpy() for key in FIELDS}
    ref = {key: getattr(ch_m, key).numpy() for key in FIELDS + ("status",)}
    ref.update(bound_avk=bounds["bound_avk"], bound_diag=bounds["bound_diag"])
    return ncr.char_errors(got, ref, dict(sa=np.asarray(sa)))


def same_rows(ch_n, ch_m):
    return ch_n.status.tolist() == ch_m.status.tolist() and ch_n.nobs.tolist() == ch_m.nobs.tolist() and torch.equal(ch_n.keep, ch_m.keep)


def test_with_form_m_nothing_reaches_the_new_seams(monkeypatch):
    st = NfCharStandins(monkeypatch)
    s = setup()
    ov = make(s)
    y = observations(st, s)
    ov.characterise(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    assert st.nf_chars == [] and st.nf_gains == [] and st.nf_prepares == []
    with pytest.raises(ValueError, match="characterise_nform needs form='n'"):
        ov.characterise_nform(s["z"], s["p"], s["x_true"], y)
    with pytest.raises(ValueError, match="characterise_nform"):          # ... and the other way round, the message names it
        make(s, form="n").characterise(s["z"], s["p"], s["x_true"], y)


def test_characterise_nform_equals_characterise_of_the_twin(monkeypatch):
    st = NfCharStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    y[1, 0, 2] = float("nan")                                            # one observation missing
    ov_m, ov_n = pair(s)
    ch_m = ov_m.characterise(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    gains, k_calls = len(st.gain_calls), len(st.k_calls)
    st.order.clear()
    ch_n = ov_n.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    assert isinstance(ch_n, retrieval.Characterisation) and ch_n.coeff is None
    assert len(st.k_calls) == k_calls + 1 and len(st.gain_calls) == gains and st.nf_solves == []     # one K-matrix call, no m-form gain
    assert len(st.nf_prepares) == 1 and st.order == ["nform_char", "nform_gain"]
    assert st.nf_prepares[0]["se"] is ov_n.se and st.nf_gains[0]["se"] is ov_n.se and st.nf_chars[0]["nblk"] == 2
    assert st.nf_chars[0]["asked"] == ["avk", "avk_diag", "dfs_block", "noise_var", "post_cov", "smooth_var", "status"]
    assert st.nf_chars[0]["rows"] == (0, 0)
    assert same_rows(ch_n, ch_m) and ch_n.nobs.tolist() == [M, M - 1, M] and (ch_n.gain[1, 2] == 0).all()
    assert ch_n.gain.shape == (NPROF, M, N) and ch_n.avk.shape == ch_n.post_cov.shape == (NPROF, N, N)
    err = char_errors(ch_n, ch_m, st.nf_chars[0]["ref"], s["sa"])
    assert set(err) == set(FIELDS) and max(err.values()) <= BAR, err


def test_gain_false_and_the_row_window(monkeypatch):
    st = NfCharStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    ov = make(s, form="n")
    full = ov.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    bare = ov.characterise_nform(s["z"], s["p"], s["x_true"], y, gain=False)
    assert bare.gain is None and bare.avk is None and bare.post_cov is None and len(st.nf_gains) == 1
    assert st.nf_chars[-1]["asked"] == ["avk_diag", "dfs_block", "noise_var", "smooth_var", "status"]       # S^ stays in the kernel
    for key in ("avk_diag", "dfs_block", "noise_var", "smooth_var", "status", "nobs", "keep"):
        assert torch.equal(getattr(bare, key), getattr(full, key)), key
    win = ov.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, rows=(NLEV - 1, 3))
    assert st.nf_chars[-1]["rows"] == (NLEV - 1, 3) and win.avk.shape == win.post_cov.shape == (NPROF, 3, N)
    assert torch.equal(win.avk, full.avk[:, NLEV - 1:NLEV + 2]) and torch.equal(win.post_cov, full.post_cov[:, NLEV - 1:NLEV + 2])
    assert torch.equal(win.gain, full.gain)                              # the gain is formed from the full S^
    only = ov.characterise_nform(s["z"], s["p"], s["x_true"], y, gain=False, post_cov=True, rows=(2, 1))
    assert only.post_cov.shape == (NPROF, 1, N) and torch.equal(only.post_cov, full.post_cov[:, 2:3]) and len(st.nf_gains) == 2
    for bad in ((-1, 2), (0, 0), (N - 1, 2), (N, 1)):
        with pytest.raises(ValueError, match="rows: expected"):
            ov.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, rows=bad)


def test_with_a_basis_everything_is_in_coefficient_space(monkeypatch):
    st = NfCharStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    sb = eofs(s)
    ov_m, ov_n = pair(s, basis=sb)
    c = torch.as_tensor(np.random.default_rng(3).standard_normal((NPROF, R)) * 0.2)
    ch_m = ov_m.characterise(s["z"], s["p"], c, y, avk=True, post_cov=True)
    ch_n = ov_n.characterise_nform(s["z"], s["p"], c, y, avk=True, post_cov=True)
    assert [tuple(k.shape) for k in st.nf_gains[0]["k"]] == [(NPROF, M, R)] and st.nf_chars[0]["nblk"] == 1
    assert ch_n.gain.shape == (NPROF, M, R) and ch_n.avk.shape == (NPROF, R, R) and ch_n.avk_diag.shape == (NPROF, 1, R)
    assert ch_n.dfs_block.shape == (NPROF, 1) and torch.equal(ch_n.coeff, c) and same_rows(ch_n, ch_m)
    err = char_errors(ch_n, ch_m, st.nf_chars[0]["ref"], sb.sa_c.numpy())
    assert max(err.values()) <= BAR, err


def test_with_an_instrument_the_rows_are_channel_rows(monkeypatch):
    st = NfCharStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    inst = Instrument(FRQ, ELEV, beam=3.5, band=0.23, n_beam=3, n_band=2)
    ov_m, ov_n = pair(s, instrument=inst)
    ch_m = ov_m.characterise(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    ch_n = ov_n.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    assert [tuple(k.shape) for k in st.nf_gains[0]["k"]] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2 and same_rows(ch_n, ch_m)
    assert max(char_errors(ch_n, ch_m, st.nf_chars[0]["ref"], s["sa"]).values()) <= BAR


def test_per_profile_se_in_both_shapes(monkeypatch):
    st = NfCharStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    y[2, 1, 0] = float("nan")
    ov_m, ov_n = pair(s)
    var = torch.as_tensor(0.25 * (1.0 + np.random.default_rng(8).uniform(0.0, 2.0, (NPROF, M))))
    ch_m = ov_m.characterise(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, se=var)       # the m-form whitens
    whitens, applies = len(st.whiten_calls), len(st.apply_calls)
    ch_n = ov_n.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, se=var)
    # [nprof][m] goes straight in: nothing is whitened, nothing to undo
    assert (len(st.whiten_calls), len(st.apply_calls)) == (whitens, applies) == (1, 1)
    assert torch.equal(st.nf_prepares[-1]["se"], var) and torch.equal(st.nf_gains[-1]["se"], var) and same_rows(ch_n, ch_m)
    assert max(char_errors(ch_n, ch_m, st.nf_chars[-1]["ref"], s["sa"]).values()) <= BAR
    # [nprof][m][m] goes through the pre-whitening, then variances of 1; the gain is un-whitened after everything else
    full = se_batch()
    ch_m = ov_m.characterise(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, se=full)
    st.order.clear()
    ch_n = ov_n.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, se=full)
    assert st.order == ["whiten", "nform_char", "nform_gain", "apply1"] and st.apply_calls[-1]["mode"] == 1
    assert (st.nf_gains[-1]["se"] == 1.0).all() and st.nf_gains[-1]["se"].shape == (M,)
    assert st.nf_gains[-1]["k"][0] is st.whiten_calls[-1]["out"]["k"][0] and same_rows(ch_n, ch_m)
    assert (ch_n.gain[2, 3] == 0).all()                                  # row (1, 0) of profile 2 was dropped
    assert max(char_errors(ch_n, ch_m, st.nf_chars[-1]["ref"], s["sa"]).values()) <= BAR
    # an indefinite Se_p: status 2 and NaN in every floating-point field, as with form="m"
    bad = full.clone()
    bad[1] = -bad[1]
    ch = ov_n.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, se=bad)
    assert ch.status.tolist() == [1, 2, 1] and ch.nobs.tolist() == [M, 0, M - 1]
    for key in FIELDS:
        assert torch.isnan(getattr(ch, key)[1]).all() and torch.isfinite(getattr(ch, key)[[0, 2]]).all(), key


def test_failed_and_unobserved_profiles(monkeypatch):
    NfCharStandins(monkeypatch)
    s = setup()
    ov = make(s, form="n")
    y = torch.full((NPROF, ELEV.size, FRQ.size), 255.0, dtype=torch.float64)
    y[1] = float("nan")                                                  # nothing observed: the prior
    x = s["x_true"].clone()
    x[0, 1, 2] = float("nan")                                            # a state that is not finite
    ch = ov.characterise_nform(s["z"], s["p"], x, y, avk=True, post_cov=True, rows=(1, 4))
    assert ch.status.tolist() == [0, 3, 1] and ch.nobs.tolist() == [0, 0, M]
    for key in FIELDS:
        assert torch.isnan(getattr(ch, key)[0]).all(), key
    for key in ("gain", "avk", "avk_diag", "dfs_block", "noise_var"):
        assert (getattr(ch, key)[1] == 0).all(), key
    assert (ch.post_cov[1] - ov.sa[1:5]).abs().max() <= BAR * ov.sa.abs().max() and ch.avk.shape == (NPROF, 4, N)


def test_more_observations_than_the_m_form_takes(monkeypatch):
    """14 channels x 11 elevations = 154 observations: characterise refuses through its entry's limit, this one runs."""
    st = NfCharStandins(monkeypatch)
    s = setup()
    frq, elev = np.linspace(22.0, 58.0, 14), np.linspace(10.0, 90.0, 11)
    m = frq.size * elev.size
    assert m == 154
    ov = retrieval.OneDVar("R24", frq, elev, torch.as_tensor(s["sa"]), torch.full((m,), 0.25, dtype=torch.float64),
                           variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=torch.as_tensor(s["xa"]), form="n")
    y = st.forward(s["x_true"][:, 0], s["x_true"][:, 1], frq, elev).reshape(NPROF, elev.size, frq.size)
    ch = ov.characterise_nform(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True)
    assert ch.status.tolist() == [1] * NPROF and ch.nobs.tolist() == [m] * NPROF and ch.gain.shape == (NPROF, m, N)
    rows = st.rows(frq, elev)
    K = np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)
    post = np.linalg.inv(K.T @ K / 0.25 + np.linalg.inv(s["sa"]))
    gain = (post @ K.T / 0.25).T
    assert np.abs(ch.post_cov[0].numpy() - post).max() <= BAR * np.abs(post).max()
    assert np.abs(ch.gain[0].numpy() - gain).max() <= BAR * np.abs(gain).max()
    assert np.abs(ch.avk[0].numpy() - gain.T @ K).max() <= BAR * (np.abs(gain).T @ np.abs(K)).max()
    assert abs(float(ch.dfs_block[0].sum()) - np.trace(gain.T @ K)) <= BAR * max(1.0, np.trace(gain.T @ K))
