"""retrieval.OneDVar(..., ray_tracing=True) without a GPU: the stand-ins of tests/test_retrieval_instrument_cpu.py replace
the seams to the native library, and a second K-matrix stand-in sits on the ray seam.  What is checked is which seam the
module reaches: with ``ray_tracing=True`` every forward run goes through ``_native_k_matrix_ray`` (twelve positional
parameters, as ``_native_k_matrix``) and never through ``_native_k_matrix``; the default does the reverse; and with an
instrument the ray seam is asked for the instrument's quadrature grid."""
import inspect

import pytest

torch = pytest.importorskip("torch")

import test_retrieval_instrument_cpu as tri  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402


class RayStandins(tri.Standins):
    """tri.Standins plus the same linear model on the ray seam, with its own call log."""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.ray_calls = []
        monkeypatch.setattr(retrieval, "_native_k_matrix_ray", self.k_matrix_ray)

    def k_matrix_ray(self, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
        n = len(self.k_calls)
        out = self.k_matrix(model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream)
        self.ray_calls.append(self.k_calls.pop())
        assert len(self.k_calls) == n
        return out


def test_the_two_seams_take_the_same_twelve_parameters():
    a = list(inspect.signature(retrieval._native_k_matrix).parameters)
    b = list(inspect.signature(retrieval._native_k_matrix_ray).parameters)
    assert a == b and len(a) == 12


def test_ray_tracing_reaches_the_ray_seam_only(monkeypatch):
    st = RayStandins(monkeypatch)
    s = tri.setup()
    ov = tri.make(s, ray_tracing=True)
    y = torch.full((tri.NPROF, tri.ELEV.size, tri.FRQ.size), 255.0, dtype=torch.float64)
    ov.step(s["z"], s["p"], s["x_true"], y)
    ov.forward(s["z"], s["p"], s["x_true"])
    ov.retrieve(s["z"], s["p"], y, max_iter=2)
    ov._linearise(s["z"], s["p"], s["x_true"])              # what retrieve_lm and characterise linearise with
    assert st.k_calls == [] and len(st.ray_calls) >= 4
    for call in st.ray_calls:
        model, z, p, t, rh, dl, di, frq, elev, variables, want, stream = call["args"]
        assert model == "R24" and frq is ov.frq and elev is ov.elev and variables is ov.variables and want == ("t", "h")
        assert dl is None and di is None and stream is None


def test_the_default_never_reaches_the_ray_seam(monkeypatch):
    st = RayStandins(monkeypatch)
    s = tri.setup()
    ov = tri.make(s)
    assert ov.ray_tracing is False
    y = torch.full((tri.NPROF, tri.ELEV.size, tri.FRQ.size), 255.0, dtype=torch.float64)
    ov.step(s["z"], s["p"], s["x_true"], y)
    ov.forward(s["z"], s["p"], s["x_true"])
    assert st.ray_calls == [] and len(st.k_calls) == 2


def test_with_an_instrument_the_ray_seam_is_asked_for_the_quadrature_grid(monkeypatch):
    st = RayStandins(monkeypatch)
    s = tri.setup()
    inst = Instrument(tri.FRQ, tri.ELEV, beam=3.5, band=[0.23, 0.23, 2.0], n_beam=3, n_band=2)
    ov = tri.make(dict(s, se=s["se"][:inst.m_out]), instrument=inst, ray_tracing=True)
    y = torch.full((tri.NPROF, inst.elev.size, inst.frq.size), 255.0, dtype=torch.float64)
    ov.step(s["z"], s["p"], s["x_true"], y)
    assert st.k_calls == [] and len(st.ray_calls) == 1 and len(st.obs_calls) == 1
    args = st.ray_calls[0]["args"]
    assert args[7] is inst.frq_q and args[8] is inst.elev_q and args[10] == ("t", "h")
    # the update saw channel rows: the reduction ran on what the ray seam returned
    assert st.step_calls[0]["k"][0].shape == (tri.NPROF, inst.elev.size, inst.frq.size, tri.NLEV)
