"""The tensor contract of retrieval.py (its module docstring) through the real library on the GPU: every
tensor argument in an awkward but valid layout at once gives, bit for bit, what contiguous clones give (the same kernels on
the same numbers), and what the contract refuses is refused before a context is asked for.  3 profiles, 8 levels, 3
frequencies x 2 elevations, a basis of r = 4, a two-point-per-channel instrument.

tests/test_tensor_contract_cpu.py is what shows that no bad pointer is left to hand over; the layouts here are those whose
storage holds at least the contiguous extent behind the view's own pointer (slices of larger buffers, permuted storage,
offsets with room behind), so that even a missed ``.contiguous()`` would read wrong numbers, not foreign memory.  No
tolerance appears in this file."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NPROF, NLEV, R = 3, 8, 4
FRQ = np.array([22.24, 31.4, 53.86])
ELEV = np.array([90.0, 19.2])
M = FRQ.size * ELEV.size


def every_other(t):
    buf = torch.full(t.shape[:-1] + (2 * t.shape[-1],), -7.0, dtype=t.dtype, device=t.device)
    buf[..., ::2] = t
    return buf[..., ::2]


def permuted(t):
    """Stored with the first two axes swapped: z held as [nlev][nprof], x as [nblk][nprof][nlev], sa as sa.T."""
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def offset(t):
    buf = torch.full((t.numel() + 5,), -7.0, dtype=t.dtype, device=t.device)
    buf[3:3 + t.numel()] = t.reshape(-1)
    return buf[3:3 + t.numel()].view(t.shape)


def awkward(tensors):
    """Every tensor of a dict in another layout, the three kinds rotating over the names (1-D: no permutation)."""
    out = {}
    for i, (name, t) in enumerate(sorted(tensors.items())):
        kinds = [every_other, offset] + ([permuted] if t.dim() >= 2 else [])
        out[name] = kinds[i % len(kinds)](t)
        assert np.array_equal(out[name].cpu().numpy(), t.cpu().numpy(), equal_nan=True), name
        assert not (out[name].is_contiguous() and out[name].storage_offset() == 0), name
        assert out[name].untyped_storage().nbytes() // 8 - out[name].storage_offset() >= t.numel(), name
    return out


def numbers():
    """The well-formed inputs, contiguous CUDA tensors by name."""
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr
    from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    P = pr.synthetic_profiles(NPROF, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, NLEV)).astype(int)
    z, p, t, rh = (dev(P[k][:, pick]) for k in ("z", "p", "t", "rh"))
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 3.0)
    sa = np.zeros((2 * NLEV, 2 * NLEV))
    for b, sig in enumerate((2.0, 0.05)):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig ** 2 * corr
    rng = np.random.default_rng(23)
    xa = torch.stack([t, rh], dim=1).contiguous()                        # a prior per profile
    x = (xa + dev(rng.standard_normal((NPROF, 2, NLEV)) * np.array([1.0, 0.02])[None, :, None])).clamp(min=1e-3)
    eof = StateBasis.from_covariance(torch.as_tensor(sa), R)
    j = rng.standard_normal((NPROF, M, 3)) * 0.3
    se_p = (0.1 + 0.2 * np.arange(NPROF))[:, None, None] * np.eye(M) + j @ j.transpose(0, 2, 1)
    return dict(z=z, p=p, x=x, x0=xa + 0.1 * (x - xa), sa=dev(sa), se=dev(np.full(M, 0.25)), xa=xa, b=dev(eof.b.numpy()),
                sa_c=dev(eof.sa_c.numpy()), c_a=dev(0.2 * rng.standard_normal((NPROF, R))), c=dev(0.5 * rng.standard_normal((NPROF, R))),
                se_p=dev(se_p), noise=dev(0.3 * rng.standard_normal((NPROF, ELEV.size, FRQ.size))))


def build(t, **kw):
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    if kw.pop("basis", False):
        kw["basis"] = retrieval.StateBasis(t["b"], t["sa_c"], t["c_a"])
    return retrieval.OneDVar("R24", FRQ, ELEV, None if "basis" in kw else t["sa"], t["se"], variables=JacVariables.of(humidity="rh"),
                             blocks=("t", "h"), xa=t["xa"], **kw)


def fields(res, prefix=""):
    if res is None or torch.is_tensor(res):
        return {prefix: res}
    if dataclasses.is_dataclass(res):
        res = vars(res)
    items = res.items() if isinstance(res, dict) else enumerate(res)
    return {k: v for key, part in items for k, v in fields(part, f"{prefix}.{key}").items()}


def differing(got, want):
    got, want = fields(got), fields(want)
    bad = sorted(set(got) ^ set(want))
    for key in set(got) & set(want):
        g, w = got[key], want[key]
        if (g is None) != (w is None) or (g is not None and (g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(
                g.cpu().numpy(), w.cpu().numpy(), equal_nan=g.is_floating_point()))):
            bad.append(key)
    return bad


def both_layouts(run, **kw):
    """``run(ov, t)`` on contiguous clones and with every tensor awkward at once -> (the two results' differing fields, the
    contiguous result)."""
    good = numbers()
    ov = build(good, **kw)
    good["y"] = ov.forward(good["z"], good["p"], good["x"])[0] + good["noise"]
    good["y"][1, 1, 2] = float("nan")                                    # one observation missing
    want = run(ov, good)
    odd = awkward(good)
    got = run(build(odd, **kw), odd)
    torch.cuda.synchronize()
    return differing(got, want), want


def test_m_form_takes_any_layout(gpu_ctx):
    bad, want = both_layouts(lambda ov, t: dict(
        step=ov.step(t["z"], t["p"], t["x"], t["y"]),
        retrieve=ov.retrieve(t["z"], t["p"], t["y"], x0=t["x0"], max_iter=3),
        retrieve_lm=ov.retrieve_lm(t["z"], t["p"], t["y"], x0=t["x0"], max_iter=3),
        characterise=ov.characterise(t["z"], t["p"], t["x"], t["y"], avk=True, post_cov=True)))
    assert bad == []
    assert want["step"][1]["status"].cpu().tolist() == [1] * NPROF and want["characterise"].status.cpu().tolist() == [1] * NPROF
    assert want["step"][1]["nobs"].cpu().tolist() == [M, M - 1, M] and bool(torch.isfinite(want["retrieve_lm"].x).all())


def test_n_form_with_a_basis_takes_any_layout(gpu_ctx):
    bad, want = both_layouts(lambda ov, t: dict(
        step=ov.step(t["z"], t["p"], t["c"], t["y"], post_cov=True),
        retrieve_lm=ov.retrieve_lm(t["z"], t["p"], t["y"], x0=t["c"], max_iter=3),
        characterise=ov.characterise_nform(t["z"], t["p"], t["c"], t["y"], avk=True, post_cov=True)), basis=True, form="n")
    assert bad == []
    assert want["step"][1]["status"].cpu().tolist() == [1] * NPROF and want["characterise"].status.cpu().tolist() == [1] * NPROF
    assert want["step"][1]["post_cov"].shape == (NPROF, R, R) and bool(torch.isfinite(want["retrieve_lm"].x).all())


def test_an_instrument_with_a_full_per_profile_se_takes_any_layout(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument
    bad, want = both_layouts(lambda ov, t: dict(
        step=ov.step(t["z"], t["p"], t["x"], t["y"], se=t["se_p"]),
        characterise=ov.characterise(t["z"], t["p"], t["x"], t["y"], se=t["se_p"])),
        instrument=Instrument(FRQ, ELEV, band=([-0.1, 0.1], [0.5, 0.5])))
    assert bad == []
    assert want["step"][1]["whiten_status"].cpu().tolist() == [1] * NPROF and want["characterise"].status.cpu().tolist() == [1] * NPROF


def test_what_the_contract_refuses_never_asks_for_a_context(gpu_ctx, monkeypatch):
    from mwr_fast_forward_operators_and_lbls_amd import _native
    t = numbers()
    ov = build(t)
    y = ov.forward(t["z"], t["p"], t["x"])[0]
    torch.cuda.synchronize()

    def no_context(device_id=0):
        raise AssertionError("a refused argument got as far as asking for a context")
    monkeypatch.setattr(_native, "default_context", no_context)
    for name, bad in (("p", t["p"].cpu()), ("x", t["x"].to(torch.float32)), ("y", y.cpu()), ("z", t["z"].to(torch.float32))):
        args = dict(z=t["z"], p=t["p"], x=t["x"], y=y)
        args[name] = bad
        for call in (lambda a: ov.step(a["z"], a["p"], a["x"], a["y"]), lambda a: ov.retrieve(a["z"], a["p"], a["y"], x0=a["x"]),
                     lambda a: ov.retrieve_lm(a["z"], a["p"], a["y"], x0=a["x"]),
                     lambda a: ov.characterise(a["z"], a["p"], a["x"], a["y"])):
            with pytest.raises(ValueError, match=rf"^(x0|{name}):"):
                call(args)
    with pytest.raises(ValueError, match="^sa:"):
        build(dict(t, sa=t["sa"].cpu()))
    with pytest.raises(ValueError, match="^se:"):
        build(dict(t, se=t["se"].to(torch.float32)))
    other = build(dict(t, xa=torch.cat([t["xa"], t["xa"][-1:]], dim=0)))       # a per-profile prior of another batch size
    for call in (lambda: other.step(t["z"], t["p"], t["x"], y), lambda: other.retrieve(t["z"], t["p"], y),
                 lambda: other.characterise(t["z"], t["p"], t["x"], y), lambda: other.forward(t["z"], t["p"], t["x"])):
        with pytest.raises(ValueError, match="^xa:"):
            call()
