"""Host logic of the sensitivity module without a GPU: parameter names, relative scaling and K_b S_b K_b^T, with a stand-in
for the one native call (defined here; the product code has no alternative engine)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd import _native, sensitivity, spectroscopy as sp  # noqa: E402


def test_parse_params_names_lines_and_expansion():
    m = sp.get_model("R20")
    recs = sensitivity.parse_params(m, ["h2o_w0[0]", "o2_w300[*]", "h2o_cf", " o2_y0[ 3 ] "])
    assert [(q.name, q.line) for q in recs] == [("h2o_w0", 0), ("o2_w300", -1), ("h2o_cf", 0), ("o2_y0", 3)]
    assert [q.field for q in recs] == [_native.PARAM_FIELDS[n] for n in ("h2o_w0", "o2_w300", "h2o_cf", "o2_y0")]
    assert recs[0].value == m.h2o["w0"][0] and recs[1].value == 1.0 and recs[2].value == m.h2o_cf and recs[3].value == m.o2["y0"][3]
    assert [q.label for q in recs] == ["h2o_w0[0]", "o2_w300[*]", "h2o_cf", "o2_y0[3]"]
    # a bare per-line name: every line of the model, in order
    full = sensitivity.parse_params("R20", ["o2_s300", "n2_l"])
    n = len(m.o2["f"])
    assert len(full) == n + 1 and [q.line for q in full[:n]] == list(range(n)) and full[-1].name == "n2_l"
    assert [q.value for q in full[:n]] == [float(x) for x in m.o2["s300"]]
    # every field of the ABI has a name, and the scalars sit below the per-line fields
    assert len(_native.PARAM_FIELDS) == 24 and sorted(_native.PARAM_FIELDS.values()) == list(range(24))
    for name, fid in _native.PARAM_FIELDS.items():
        per_line = name.split("_", 1)[1] in (m.h2o if name.startswith("h2o") else m.o2) and not hasattr(m, name)
        assert per_line == (fid >= _native.PAR_FIRST_H2O_LINE_FIELD), name


@pytest.mark.parametrize("bad", [["h2o_fl[0]"], ["h2o_cf[0]"], ["o2_x[*]"], ["h2o_w0[99]"], ["o2_y0[-1]"], ["h2o_w0[0"], [],
                                 ["o2_s300"] * 6, [3]])
def test_parse_params_refusals(bad):
    with pytest.raises(ValueError):
        sensitivity.parse_params("R20", bad)


def stand_in(tables, z, p, t, rh, frq, elev, recs):
    """kb[i, a, j, q] = (q + 1) * (1 + i) * frq[j] / elev[a]: a known array in the native layout."""
    i = torch.arange(z.shape[0], dtype=torch.float64)[:, None, None, None] + 1.0
    a = 1.0 / torch.tensor(elev)[None, :, None, None]
    j = torch.tensor(frq)[None, None, :, None]
    q = torch.arange(len(recs), dtype=torch.float64)[None, None, None, :] + 1.0
    kb = i * a * j * q
    return kb.sum(-1), kb, torch.ones(z.shape[0], dtype=torch.uint8)


def test_relative_scaling_and_argument_checks(monkeypatch):
    monkeypatch.setattr(sensitivity, "_native_param_jacobian", stand_in)
    m = sp.get_model("R17")
    prof = [torch.ones((2, 5), dtype=torch.float64) for _ in range(4)]
    specs = ["h2o_w0[1]", "o2_w300[*]", "o2_x"]
    tb, kb, valid = sensitivity.param_jacobian(m, *prof, [22.0, 31.0], [90.0], specs)
    tb_r, kb_r, _ = sensitivity.param_jacobian(m, *prof, [22.0, 31.0], [90.0], specs, relative=True)
    assert kb.shape == (2, 1, 2, 3) and torch.equal(tb, tb_r)
    scale = torch.tensor([m.h2o["w0"][1], 1.0, m.o2_x], dtype=torch.float64)
    assert torch.equal(kb_r, kb * scale)
    # records are taken as they are
    recs = sensitivity.parse_params(m, specs)
    assert torch.equal(sensitivity.param_jacobian(m, *prof, [22.0, 31.0], [90.0], recs)[1], kb)
    with pytest.raises(ValueError):
        sensitivity.param_jacobian(m, prof[0], prof[1], prof[2], prof[3].float(), [22.0], [90.0], specs)
    with pytest.raises(ValueError):
        sensitivity.param_jacobian(m, prof[0], prof[1], prof[2], prof[3][:, :4], [22.0], [90.0], specs)


def test_the_native_path_refuses_cpu_tensors():
    prof = [torch.ones((1, 5), dtype=torch.float64) for _ in range(4)]
    with pytest.raises(ValueError, match="CUDA"):
        sensitivity.param_jacobian("R17", *prof, [22.0], [90.0], ["h2o_cf"])


def test_model_error_covariance_against_einsum(monkeypatch):
    rng = np.random.default_rng(0)
    kb = torch.tensor(rng.normal(size=(3, 2, 4, 5)))
    k = kb.numpy().reshape(3, 8, 5)
    var = rng.uniform(0.1, 2.0, 5)
    A = rng.normal(size=(5, 5))
    full = A @ A.T
    for sb, ref in ((var, np.einsum("pik,k,pjk->pij", k, var, k)), (full, np.einsum("pik,kl,pjl->pij", k, full, k))):
        cov = sensitivity.model_error_covariance(kb, sb).numpy()
        assert cov.shape == (3, 8, 8) and np.abs(cov - ref).max() <= 1e-13 * np.abs(ref).max()
        assert np.array_equal(cov, cov.transpose(0, 2, 1))
        assert all(np.linalg.eigvalsh(c).min() >= -1e-12 * np.abs(c).max() for c in cov)
        mean = sensitivity.model_error_covariance(kb, sb, reduce="mean").numpy()
        assert mean.shape == (8, 8) and np.abs(mean - ref.mean(axis=0)).max() <= 1e-13 * np.abs(ref).max()
    # [nprof][m][npar] is taken as it is
    assert torch.equal(sensitivity.model_error_covariance(kb.reshape(3, 8, 5), var), sensitivity.model_error_covariance(kb, var))
    for bad in (np.ones(4), np.ones((5, 4))):
        with pytest.raises(ValueError):
            sensitivity.model_error_covariance(kb, bad)
    with pytest.raises(ValueError):
        sensitivity.model_error_covariance(kb, var, reduce="sum")
