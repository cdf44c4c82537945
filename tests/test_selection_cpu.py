"""selection.select_observations and selection.rank_observations without a GPU: the seams of retrieval are replaced as in
tests/test_retrieval_nform_cpu.py and the one new seam, ``selection._native_oe_select``, by the longdouble reference of
tests/select_reference.py.  What is checked is the module's own work: what reaches the seam for both forms, with a basis,
with an instrument and with ``se=`` per profile; the derived fields of ``Selection``; the refusals, by message; and that the
``form="m"`` and ``form="n"`` twins of one retrieval give the same ``Selection``."""
import numpy as np
import pytest

import select_reference as sr

torch = pytest.importorskip("torch")

import mwr_fast_forward_operators_and_lbls_amd as pkg  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import retrieval, selection  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402
from test_retrieval_basis_cpu import N, R, eofs  # noqa: E402
from test_retrieval_instrument_cpu import ELEV, FRQ, M, NLEV, NPROF, make, setup  # noqa: E402
from test_retrieval_nform_cpu import NfStandins  # noqa: E402
from test_retrieval_se_cpu import se_batch  # noqa: E402


class SelStandins(NfStandins):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.select_calls = []
        monkeypatch.setattr(selection, "_native_oe_select", self.oe_select)

    def oe_select(self, k_blocks, se, s0, nsel, keep, candidate, sa_inv, out, stream):
        self.select_calls.append(dict(k=list(k_blocks), se=se, s0=s0, nsel=nsel, keep=keep, candidate=candidate, sa_inv=sa_inv,
                                      asked=sorted(out), stream=stream))
        assert all(k.is_contiguous() and k.dim() == 3 for k in k_blocks) and se.is_contiguous() and s0.is_contiguous()
        nprof, m, nlev = k_blocks[0].shape
        for i in range(nprof):
            K = np.concatenate([k[i].numpy() for k in k_blocks], axis=1)
            r = sr.select_reference(K, (se[i] if se.dim() == 2 else se).numpy(), (s0[i] if s0.dim() == 3 else s0).numpy(), nsel,
                                    None if keep is None else keep[i].numpy(), None if candidate is None else candidate.numpy(),
                                    None if sa_inv is None else sa_inv.numpy())
            out["order"][i], out["q_pick"][i] = torch.as_tensor(r["order"]), torch.as_tensor(r["q"])
            out["rank"][i], out["q"][i] = torch.as_tensor(r["rank"]), torch.as_tensor(r["q_left"])
            out["count"][i], out["status"][i] = int(r["count"]), int(r["status"])
            S = r["S"].astype(np.float64)
            for key, v in (("dfs_gain", r["dfs_gain"]), ("post_cov", S), ("post_var", np.diag(S))):
                if key in out:
                    out[key][i] = torch.as_tensor(np.ascontiguousarray(v)).reshape(out[key][i].shape)


def same(a, b, tol=0.0):
    for key in ("order", "rank", "count", "status"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    for key in ("q", "info_bits", "cum_info", "dfs_gain", "cum_dfs", "q_left", "post_var"):
        x, y = getattr(a, key), getattr(b, key)
        assert (x is None) == (y is None), key
        if x is not None:
            assert float((x - y).abs().max()) <= tol * max(1.0, float(y.abs().max())), key


def test_the_package_exports_the_module():
    assert pkg.rank_observations is selection.rank_observations and pkg.select_observations is selection.select_observations
    assert pkg.Selection is selection.Selection and set(pkg.__all__) >= {"Selection", "select_observations", "rank_observations"}
    assert "selection" in retrieval.__doc__


def test_both_forms_give_the_same_selection(monkeypatch):
    st = SelStandins(monkeypatch)
    s = setup()
    ov_m, ov_n = make(s), make(s, form="n")
    sel_m = selection.rank_observations(ov_m, s["z"], s["p"], s["x_true"])
    sel_n = selection.rank_observations(ov_n, s["z"], s["p"], s["x_true"])
    same(sel_m, sel_n)
    assert len(st.select_calls) == 2 and len(st.k_calls) == 2           # one K-matrix call each, nothing else
    assert st.step_calls == [] and st.nf_prepares == [] and st.gain_calls == []
    c = st.select_calls[0]
    assert [tuple(k.shape) for k in c["k"]] == [(NPROF, M, NLEV)] * 2 and c["nsel"] == M and c["keep"] is None
    assert c["se"] is ov_m.se and c["s0"] is ov_m.sa and c["sa_inv"] is ov_m.sa_inv and c["candidate"] is None
    assert c["asked"] == ["count", "dfs_gain", "order", "post_var", "q", "q_pick", "rank", "status"]
    rows = st.rows(FRQ, ELEV)
    assert torch.equal(c["k"][0][0], rows["t"]) and torch.equal(c["k"][1][2], rows["h"])
    # the fields: all M picked, the bits and the running sums, the layout of the scan
    assert sel_m.order.shape == (NPROF, M) and sel_m.count.tolist() == [M] * NPROF and sel_m.status.tolist() == [1] * NPROF
    assert sorted(sel_m.order[0].tolist()) == list(range(M)) and sel_m.nf == FRQ.size
    assert torch.equal(sel_m.info_bits, 0.5 * torch.log2(1.0 + sel_m.q)) and torch.equal(sel_m.cum_info, sel_m.info_bits.cumsum(1))
    assert torch.equal(sel_m.cum_dfs, sel_m.dfs_gain.cumsum(1)) and sel_m.post_cov is None
    assert torch.equal(sel_m.elev_index, sel_m.order // FRQ.size) and torch.equal(sel_m.freq_index, sel_m.order % FRQ.size)
    assert torch.equal(sel_m.rank.gather(1, sel_m.order.long()), torch.arange(M, dtype=torch.int32).expand(NPROF, M))
    # all picked: the dfs is that of the full update, and post_var its posterior's diagonal
    K = np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)
    post = np.linalg.inv(K.T @ K / 0.25 + np.linalg.inv(s["sa"]))
    dfs = np.trace(np.eye(N) - post @ np.linalg.inv(s["sa"]))
    assert abs(float(sel_m.cum_dfs[0, -1]) - dfs) <= 1e-9 * N
    assert np.abs(sel_m.post_var[0].numpy().reshape(-1) - np.diag(post)).max() <= 1e-9 * np.abs(post).max()
    assert sel_m.post_var.shape == (NPROF, 2, NLEV)


def test_first_k_counts_profiles_and_minus_one_is_kept(monkeypatch):
    SelStandins(monkeypatch)
    rng = np.random.default_rng(11)
    k = torch.as_tensor(rng.standard_normal((4, 7, 3)))
    k[:, 5] = 0.0                                                        # adds nothing: never picked
    k[0, 1] *= 30.0
    sel = selection.select_observations([k], torch.full((7,), 0.5, dtype=torch.float64), torch.eye(3, dtype=torch.float64), 7, nf=2)
    assert sel.count.tolist() == [6] * 4 and (sel.order[:, -1] == -1).all() and (sel.q[:, -1] == 0).all()
    assert sel.dfs_gain is None and sel.cum_dfs is None and sel.post_var is None and (sel.info_bits[:, -1] == 0).all()
    assert (sel.elev_index[:, -1] == -1).all() and (sel.freq_index[:, -1] == -1).all()
    assert torch.equal(sel.elev_index[:, :-1], sel.order[:, :-1] // 2) and torch.equal(sel.freq_index[:, :-1], sel.order[:, :-1] % 2)
    first = sel.first(2)
    assert first.shape == (7,) and int(first.sum()) == 8 and int(first[5]) == 0 and int(first[1]) >= 1
    assert sel.first(7).tolist() == [4, 4, 4, 4, 4, 0, 4]
    with pytest.raises(ValueError, match="nf="):
        selection.select_observations([k], torch.full((7,), 0.5, dtype=torch.float64), torch.eye(3, dtype=torch.float64), 2).elev_index


def test_with_a_basis_the_selection_runs_in_coefficients(monkeypatch):
    st = SelStandins(monkeypatch)
    s = setup()
    sb = eofs(s)
    c = torch.as_tensor(np.random.default_rng(3).standard_normal((NPROF, R)) * 0.2)
    sels = [selection.rank_observations(make(s, basis=sb, form=form), s["z"], s["p"], c, nsel=4, post_cov=True) for form in "mn"]
    same(*sels)
    call = st.select_calls[0]
    assert [tuple(k.shape) for k in call["k"]] == [(NPROF, M, R)] and call["nsel"] == 4 and tuple(call["s0"].shape) == (R, R)
    assert torch.equal(call["s0"], sb.sa_c) and tuple(call["sa_inv"].shape) == (R, R) and len(st.project_calls) == 2
    assert sels[0].order.shape == (NPROF, 4) and sels[0].post_cov.shape == (NPROF, R, R) and sels[0].post_var.shape == (NPROF, 1, R)


def test_with_an_instrument_the_channel_rows_are_ranked(monkeypatch):
    st = SelStandins(monkeypatch)
    s = setup()
    inst = Instrument(FRQ, ELEV, beam=3.5, band=[0.23, 0.23, 2.0], n_beam=3, n_band=2)
    sel = selection.rank_observations(make(s, instrument=inst), s["z"], s["p"], s["x_true"], nsel=3)
    assert len(st.obs_calls) == 1 and st.k_calls[0]["args"][7] is inst.frq_q
    got = st.select_calls[0]["k"][0].numpy()
    want = inst.dense() @ st.rows(inst.frq_q, inst.elev_q)["t"].numpy()
    assert got.shape == (NPROF, M, NLEV) and np.abs(got[0] - want).max() <= 1e-13 * np.abs(want).max()
    assert sel.order.shape == (NPROF, 3)


def test_se_per_profile_and_a_candidate_mask(monkeypatch):
    st = SelStandins(monkeypatch)
    s = setup()
    ov = make(s, form="n")
    se_p = torch.as_tensor(np.random.default_rng(2).uniform(0.1, 1.0, (NPROF, M)))
    cand = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.bool)
    sel = selection.rank_observations(ov, s["z"], s["p"], s["x_true"], se=se_p, candidate=cand)
    call = st.select_calls[0]
    assert torch.equal(call["se"], se_p) and call["candidate"].dtype == torch.uint8 and call["candidate"].tolist() == [1, 1, 0, 1, 0, 1]
    assert sel.count.tolist() == [4] * NPROF and (sel.rank[:, [2, 4]] == -1).all() and (sel.q_left[:, [2, 4]] == 0).all()
    shared = selection.rank_observations(ov, s["z"], s["p"], s["x_true"], candidate=cand)
    assert not torch.equal(shared.q, sel.q)


def test_refusals_name_their_reason(monkeypatch):
    st = SelStandins(monkeypatch)
    s = setup()
    full = dict(s, se=0.25 * np.eye(M))
    with pytest.raises(ValueError, match="the constructor's se.*whitening mixes the rows.*no single observation left to rank"):
        selection.rank_observations(make(full), s["z"], s["p"], s["x_true"])
    with pytest.raises(ValueError, match="se=.*whitening mixes the rows"):
        selection.rank_observations(make(s), s["z"], s["p"], s["x_true"], se=se_batch())
    assert st.select_calls == [] and st.k_calls == []
    # a state above 128 elements: the n-form's advice
    nlev = 65
    k = [torch.zeros((2, 3, nlev), dtype=torch.float64)] * 2
    se, s0 = torch.ones(3, dtype=torch.float64), torch.eye(2 * nlev, dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 128 elements, got 130.*use a reduced basis"):
        selection.select_observations(k, se, s0, 2)
    # the tensor contract
    k = [torch.ones((2, 3, 4), dtype=torch.float64)]
    se, s0 = torch.ones(3, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
    for bad, match in ((dict(k_blocks=[k[0].float()]), r"k_blocks\[0\]: expected a float64 tensor"),
                       (dict(k_blocks=[k[0].numpy()]), r"k_blocks\[0\]: expected .* got ndarray"),
                       (dict(k_blocks=k + [torch.ones((2, 3, 5), dtype=torch.float64)]), r"k_blocks\[1\]: expected"),
                       (dict(k_blocks=[]), "1 .. 4 tensors"),
                       (dict(se=torch.ones(4, dtype=torch.float64)), r"se: expected a float64 tensor \[3\] or \[2\]\[3\]"),
                       (dict(s0=torch.eye(3, dtype=torch.float64)), r"s0: expected a float64 tensor \[4\]\[4\] or \[2\]\[4\]\[4\]"),
                       (dict(sa_inv=torch.eye(4)), "sa_inv: expected"),
                       (dict(keep=torch.ones((2, 3))), r"keep: expected a uint8 or bool tensor \[2\]\[3\]"),
                       (dict(candidate=torch.ones(2, dtype=torch.uint8)), r"candidate: expected a uint8 or bool tensor \[3\]"),
                       (dict(nsel=0), "nsel: expected an int in 1 .. 3"), (dict(nsel=4), "nsel"), (dict(nsel=2.0), "nsel")):
        args = dict(dict(k_blocks=k, se=se, s0=s0, nsel=2), **bad)
        with pytest.raises(ValueError, match=match):
            selection.select_observations(**args)
    assert st.select_calls == []
    # any strides are taken, once
    wide = torch.ones((2, 3, 8), dtype=torch.float64)[:, :, ::2]
    selection.select_observations([wide], se.expand(2, 3), s0, 2)
    assert st.select_calls[0]["k"][0].is_contiguous() and st.select_calls[0]["se"].is_contiguous()
