"""The tensor contract of retrieval.py and instrument.py (module docstring of retrieval.py) without a GPU:
the real ``_native_*`` functions run on top of tests/pointer_context.py, which takes bare integers as the library does and
checks every one of them against the tensor it came from.

  a  for well-formed inputs every route gives bit for bit what the tensor-level stand-ins of the ``*_cpu.py`` files give
     (the same NumPy code on the same numbers: a swapped buffer, a wrong flag or a wrong window shows);
  b  every context method the two modules call has an entry, every entry is called, every optional pointer is seen NULL and
     set and every flag with both values;
  c  any strides are taken: each argument in awkward but valid layouts, one at a time and all at once, gives the bits of
     contiguous clones, with no pointer the library could not read;
  d  everything else is refused with a ValueError naming the argument before any call reaches the context;
  e  CPU tensors never reach the native context.

Every comparison is bit for bit, a status value or an exception: there is no tolerance in this file."""
import dataclasses
import functools
import inspect
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_retrieval_cpu as trc  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import _native, instrument, retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis  # noqa: E402
from pointer_context import TABLE, ContractViolation, PointerContext, TensorStandins, track_pointers  # noqa: E402

NPROF, NLEV, M, R = trc.NPROF, trc.NLEV, trc.M, 4
FRQ, ELEV = trc.FRQ, trc.ELEV
ALL4 = ("t", "h", "liq", "ice")

# what each configuration switches on; every one runs every route of its form
CONFIGS = {
    "plain": {},
    "four_blocks": dict(blocks=ALL4),
    "xa_per_profile": dict(xa_per=True),
    "se_full": dict(se_full=True),
    "instrument": dict(inst=True),
    "basis": dict(basis=True, x0=True),
    "se_call_vector": dict(se_call="vector"),
    "se_call_full": dict(se_call="full", x0=True),
    "ray_tracing": dict(ray=True),
    "hydrostatic_four_blocks": dict(blocks=ALL4, heights="hydrostatic", xa_per=True, se_full=True, x0=True),
    "everything_m": dict(blocks=ALL4, xa_per=True, se_full=True, inst=True, basis=True, c_a_per=True, se_call="full", ray=True),
    "nform": dict(form="n"),
    "nform_basis": dict(form="n", basis=True, x0=True),
    "nform_se_call_vector": dict(form="n", se_call="vector", xa_per=True),
    "nform_se_call_full": dict(form="n", se_call="full"),
    "nform_basis_se_call_full": dict(form="n", basis=True, c_a_per=True, se_call="full", inst=True),
    "nform_basis_se_call_vector": dict(form="n", basis=True, se_call="vector", blocks=ALL4, xa_per=True, ray=True, x0=True),
}


def case(cfg, tweak=lambda name, t: t):
    """(ov, a) of a configuration: a fresh OneDVar and the arguments of its routes, every tensor from the same NumPy
    numbers each time.  ``tweak(name, tensor)`` may replace any of them -- the constructor's sa, se, xa, the basis' b, sa_c,
    c_a, and z, p, x, x0, y, se_call (``se=`` of a call) and x_phys (the physical state ``forward`` takes)."""
    blocks = cfg.get("blocks", ("t", "h"))
    nblk = len(blocks)
    s = trc.setup(blocks)
    rng = np.random.default_rng(17)
    t64 = lambda name, a: tweak(name, torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64))   # noqa: E731
    xa = s["xa"][None] + 0.1 * rng.standard_normal((NPROF, nblk, NLEV)) * s["sig"][None, :, None] if cfg.get("xa_per") else s["xa"]
    se = 0.25 * np.eye(M) + 0.02 if cfg.get("se_full") else s["se"]
    kw = dict(variables=JacVariables.of(humidity="rh", heights=cfg.get("heights", "fixed")), blocks=blocks,
              form=cfg.get("form", "m"), ray_tracing=cfg.get("ray", False))
    if cfg.get("inst"):
        kw["instrument"] = Instrument(FRQ, ELEV, band=([-0.1, 0.1], [0.5, 0.5]))    # two points per channel
    sa = t64("sa", s["sa"])
    if cfg.get("basis"):
        eof = StateBasis.from_covariance(torch.as_tensor(s["sa"]), R)
        c_a = 0.2 * rng.standard_normal((NPROF, R)) if cfg.get("c_a_per") else 0.1 * np.arange(R)
        kw["basis"] = StateBasis(t64("b", eof.b.numpy()), t64("sa_c", eof.sa_c.numpy()), t64("c_a", c_a))
        kw["basis"].sa_res = eof.sa_res
    ov = retrieval.OneDVar("R24", FRQ, ELEV, sa, t64("se", se), xa=t64("xa", xa), **kw)
    y = 252.0 + 2.0 * rng.standard_normal((NPROF, ELEV.size, FRQ.size))
    y[1, 1, 2] = np.nan                                                  # one observation missing
    x_phys = s["x_true"].numpy()
    x = 0.5 * rng.standard_normal((NPROF, R)) if cfg.get("basis") else x_phys
    j = rng.standard_normal((NPROF, M, 3)) * 0.3
    se_call = {None: None, "vector": 0.2 + rng.uniform(0.0, 0.3, (NPROF, M)),
               "full": (0.1 + 0.2 * np.arange(NPROF))[:, None, None] * np.eye(M) + j @ j.transpose(0, 2, 1)}[cfg.get("se_call")]
    a = types.SimpleNamespace(z=t64("z", s["z"].numpy()), p=t64("p", s["p"].numpy()), x=t64("x", x), y=t64("y", y),
                              x0=t64("x0", x + 0.01) if cfg.get("x0") else None, x_phys=t64("x_phys", x_phys),
                              se=None if se_call is None else t64("se_call", se_call))
    return ov, a


def named_tensors(cfg):
    """{name: tensor} of everything ``case`` offers to ``tweak`` in this configuration."""
    seen = {}

    def grab(name, t):
        seen[name] = t
        return t
    case(cfg, grab)
    return seen


# route -> (call, the arguments it takes, as ``tweak`` names them)
ROUTES = {
    "step": (lambda ov, a: ov.step(a.z, a.p, a.x, a.y, se=a.se, post_cov=ov.form == "n"), ("z", "p", "x", "y", "se_call")),
    "retrieve": (lambda ov, a: ov.retrieve(a.z, a.p, a.y, x0=a.x0, max_iter=3, se=a.se), ("z", "p", "y", "x0", "se_call")),
    "retrieve_lm": (lambda ov, a: ov.retrieve_lm(a.z, a.p, a.y, x0=a.x0, max_iter=3, se=a.se), ("z", "p", "y", "x0", "se_call")),
    "characterise": (lambda ov, a: ov.characterise(a.z, a.p, a.x, a.y, avk=True, post_cov=True, se=a.se),
                     ("z", "p", "x", "y", "se_call")),
    "characterise_rows": (lambda ov, a: ov.characterise(a.z, a.p, a.x, a.y, avk=True, post_cov=True, rows=(1, 2), se=a.se), ()),
    "characterise_nform": (lambda ov, a: ov.characterise_nform(a.z, a.p, a.x, a.y, avk=True, post_cov=True, se=a.se),
                           ("z", "p", "x", "y", "se_call")),
    "characterise_nform_rows": (lambda ov, a: ov.characterise_nform(a.z, a.p, a.x, a.y, gain=False, avk=True, post_cov=True,
                                                                     rows=(1, 2), se=a.se), ()),
    "forward": (lambda ov, a: ov.forward(a.z, a.p, a.x_phys), ("z", "p", "x_phys")),
    "expand": (lambda ov, a: ov.expand(a.x), ("x",)),
    "representation_error": (lambda ov, a: ov.representation_error(a.z, a.p, a.x_phys), ("z", "p", "x_phys")),
}


def routes_of(cfg):
    names = ["step", "retrieve", "retrieve_lm", "forward"]
    names += ["characterise_nform", "characterise_nform_rows"] if cfg.get("form") == "n" else ["characterise", "characterise_rows"]
    return names + (["expand", "representation_error"] if cfg.get("basis") else [])


def fields(res, prefix=""):
    """A route's result as {name: tensor or None}."""
    if res is None or torch.is_tensor(res):
        return {prefix: res}
    if dataclasses.is_dataclass(res):
        res = vars(res)
    items = res.items() if isinstance(res, dict) else enumerate(res)
    return {k: v for key, part in items for k, v in fields(part, f"{prefix}.{key}").items()}


def differing(got, want):
    """The fields in which two results differ in dtype, shape or a single bit (NaN equals NaN)."""
    got, want = fields(got), fields(want)
    bad = sorted(set(got) ^ set(want))
    for key in set(got) & set(want):
        g, w = got[key], want[key]
        if (g is None) != (w is None) or (g is not None and (
                g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g.numpy(), w.numpy(), equal_nan=g.is_floating_point()))):
            bad.append(key)
    return bad


class pointer_side:
    """``with pointer_side() as ctx``: the real ``_native_*`` functions on a ``PointerContext``."""

    def __init__(self, ctx=None):
        self.ctx, self.mp = ctx, pytest.MonkeyPatch()

    def __enter__(self):
        log = track_pointers(self.mp)
        if self.ctx is None:
            self.ctx = PointerContext(log)
        self.ctx.log = log
        self.mp.setattr(_native, "default_context", lambda device_id=0: self.ctx)
        return self.ctx

    def __exit__(self, *exc):
        self.mp.undo()


@functools.lru_cache(maxsize=None)
def sweep():
    """Every configuration and route once on each side -> ({(config, route): (pointer result, tensor result)}, context)."""
    out = {}
    with pointer_side() as ctx:
        for name, cfg in CONFIGS.items():
            ov, a = case(cfg)
            for route in routes_of(cfg):
                out[name, route] = [ROUTES[route][0](ov, a)]
        # what no configuration of OneDVar does: the instrument's reduction of K rows alone, through instrument.py
        inst = Instrument(FRQ, ELEV, band=([-0.1, 0.1], [0.5, 0.5]))
        k_q = torch.as_tensor(np.random.default_rng(2).standard_normal((NPROF, inst.elev_q.size, inst.frq_q.size, NLEV)))
        out["instrument_apply", "rows_alone"] = [inst.apply(None, [k_q])]
    with pytest.MonkeyPatch.context() as mp:
        st = TensorStandins(mp)
        for name, cfg in CONFIGS.items():
            ov, a = case(cfg)
            for route in routes_of(cfg):
                out[name, route].append(ROUTES[route][0](ov, a))
        out["instrument_apply", "rows_alone"].append(inst.apply(None, [k_q]))
        assert st.model.calls and st.ray_model.calls
    return out, ctx


# ---- a: the stand-in is faithful and the marshalling is right ------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS) + ["instrument_apply"])
def test_every_route_equals_the_tensor_level_stand_ins_bit_for_bit(config):
    results, _ = sweep()
    mine = {route: pair for (name, route), pair in results.items() if name == config and len(pair) == 2}
    assert mine and (config not in CONFIGS or sorted(mine) == sorted(routes_of(CONFIGS[config])))
    for route, (got, want) in mine.items():
        assert differing(got, want) == [], (config, route)
        assert any(v is not None and v.numel() for v in fields(got).values())


def test_the_results_are_not_trivially_equal():
    """The sweep compares numbers, not NaN with NaN: the steps succeed and the fields differ from one profile to the next."""
    results, _ = sweep()
    for (config, route), (got, _) in results.items():
        f = fields(got)
        for key, v in f.items():
            if key.endswith("status"):
                assert v.tolist() == [1] * NPROF, (config, route, key)
        floats = [v for v in f.values() if v is not None and v.is_floating_point()]
        assert all(torch.isfinite(v).any() for v in floats) and any(not torch.equal(v[0], v[1]) for v in floats), (config, route)


# ---- b: nothing is left out -----------------------------------------------------------------------------------------------
def test_every_context_method_the_modules_call_has_an_entry():
    called = set()
    for module in (retrieval, instrument):
        called |= set(re.findall(r"\.(\w+_(?:device|create|destroy))\(", inspect.getsource(module)))
    assert called and called - set(TABLE) == set(), "context methods without an entry in pointer_context.TABLE"
    assert set(TABLE) - called == set(), "entries for methods neither module calls"
    for method in TABLE:                                               # an entry describes a method the real context has
        params = inspect.signature(getattr(_native.Context, method)).parameters
        assert all(a.name in params for a in TABLE[method].args), method
        assert callable(getattr(PointerContext, method))


def test_every_entry_every_optional_pointer_and_every_flag_is_exercised():
    results, ctx = sweep()
    for method, entry in TABLE.items():
        for flag in entry.flags:
            assert len(ctx.flags[method][flag]) == 2, f"{method}: {flag} took only {ctx.flags[method][flag]}"
        for a in entry.args:
            assert "set" in ctx.seen[method][a.name], f"{method}: {a.name} never set"
    # an optional pointer the two modules never leave NULL is seen NULL here: the latest call again without it.  Nothing
    # else the call writes may change (an output does not depend on which optional outputs are asked for)
    with pointer_side(ctx):
        for method, entry in TABLE.items():
            for a in entry.args:
                if not a.optional or "null" in ctx.seen[method][a.name]:
                    continue
                tensors = [rec.tensor for rec in ctx.last[method][2].values()]
                before = [t.clone() for t in tensors]
                # (the product reads d_ksa and d_sa for the posterior covariance: without them it is the averaging kernel)
                also = dict(product=_native.OE_PRODUCT_AVK) if method == "oe_product_device" else {}
                ctx.replay(method, **{a.name: None}, **also)
                assert "null" in ctx.seen[method][a.name]
                if a.out and not also:
                    assert all(np.array_equal(t.numpy(), b.numpy(), equal_nan=True) for t, b in zip(tensors, before)), (method, a.name)
    # the handles are released with their objects
    n = ctx.calls.count("obs_destroy"), ctx.calls.count("basis_destroy")
    with pointer_side(ctx):
        ov, a = case(CONFIGS["nform_basis_se_call_full"])
        ov.step(a.z, a.p, a.x, a.y)
        ov.instrument.close()
        ov.basis.close()
    assert (ctx.calls.count("obs_destroy"), ctx.calls.count("basis_destroy")) == (n[0] + 1, n[1] + 1)
    assert set(TABLE) - set(ctx.calls) == set(), "entries no route of this file reaches"


# ---- c: layout invariance -------------------------------------------------------------------------------------------------
def expand_rows(t):
    """One shared row behind every profile: stride 0 (the rows of ``t`` must be equal)."""
    assert t.dim() >= 2 and all(torch.equal(t[0], row) for row in t)
    return t[:1].clone().expand(t.shape)


def every_other(t):
    buf = torch.full(t.shape[:-1] + (2 * t.shape[-1],), -7.0, dtype=t.dtype)
    buf[..., ::2] = t
    return buf[..., ::2]


def permuted(t):
    """Stored with the first two axes swapped: z held as [nlev][nprof], x as [nblk][nprof][nlev], sa as sa.T."""
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def offset(t):
    buf = torch.full((t.numel() + 5,), -7.0, dtype=t.dtype)
    buf[3:3 + t.numel()] = t.reshape(-1)
    return buf[3:3 + t.numel()].view(t.shape)


def layouts_of(name, t):
    kinds = [every_other, offset] + ([permuted] if t.dim() >= 2 else [])
    return kinds + ([expand_rows] if name in ("z", "p") else [])


CTOR_ARGS = ("sa", "se", "xa", "b", "sa_c", "c_a")
LAYOUT_CONFIGS = ("plain", "hydrostatic_four_blocks", "everything_m", "nform_basis_se_call_vector")


@pytest.mark.parametrize("config", LAYOUT_CONFIGS)
def test_any_layout_gives_the_bits_of_contiguous_clones(config):
    cfg = dict(CONFIGS[config], x0=True)
    shapes = named_tensors(cfg)
    with pointer_side() as ctx:
        ov, a = case(cfg)
        want = {route: ROUTES[route][0](ov, a) for route in routes_of(cfg)}

        def check(tweak, routes, what):
            assert not any(t.is_contiguous() and t.storage_offset() == 0 and t.untyped_storage().nbytes() == t.numel() * 8
                           for t in [tweak(n, shapes[n]) for n in what]), what         # the layout is an awkward one
            ov, a = case(cfg, tweak)
            for route in routes:
                try:
                    assert differing(ROUTES[route][0](ov, a), want[route]) == [], (route, what)
                except ContractViolation as err:
                    raise AssertionError(f"{route} with {what}: {err}") from err

        for route in routes_of(cfg):                                   # the arguments of each route, one at a time
            for name in ROUTES[route][1]:
                if name in shapes:
                    for kind in layouts_of(name, shapes[name]):
                        check(lambda n, t, name=name, kind=kind: kind(t) if n == name else t, [route], [name])
        for name in CTOR_ARGS:                                          # the constructors' arguments, one at a time
            if name in shapes:
                for kind in layouts_of(name, shapes[name]):
                    check(lambda n, t, name=name, kind=kind: kind(t) if n == name else t, routes_of(cfg), [name])
        for k in range(4):                                              # all at once, the layouts rotating over them
            order = sorted(shapes)
            pick = {n: layouts_of(n, shapes[n])[(i + k) % len(layouts_of(n, shapes[n]))] for i, n in enumerate(order)}
            check(lambda n, t: pick[n](t), routes_of(cfg), order)
        # a per-profile xa that is one shared state behind a stride of 0
        shared = case(dict(cfg, xa_per=False))[0].xa
        ov_c, a = case(cfg, lambda n, t: shared.expand(NPROF, -1, -1).contiguous() if n == "xa" else t)
        ov_e, a = case(cfg, lambda n, t: shared.expand(NPROF, -1, -1) if n == "xa" else t)
        for route in routes_of(cfg):
            assert differing(ROUTES[route][0](ov_e, a), ROUTES[route][0](ov_c, a)) == [], route
        assert ctx.calls


# ---- d: refusals ----------------------------------------------------------------------------------------------------------
def bad_versions(t, dim=-1):
    """What the contract refuses of a well-formed tensor ``t``: (what, the bad argument); ``dim`` is the axis that is made
    one short and one long (an axis whose size another argument states: b names r and xa names nlev themselves)."""
    yield "float32", t.to(torch.float32)
    yield "float16", t.to(torch.float16)
    yield "int64", t.to(torch.int64)
    yield "a NumPy array", t.numpy()
    yield "a list", t.tolist()
    yield "one short", t.narrow(dim, 0, t.shape[dim] - 1)
    yield "one long", torch.cat([t, t.narrow(dim, 0, 1)], dim=dim)
    yield "an extra dimension", t[None]
    yield "another device", t.to("meta")


def refused(name, call, ctx):
    shown = {"se_call": "se", "x_phys": "x", "x": "(x|c)", "prior": "(xa|c_a)"}.get(name, name)
    with pytest.raises(ValueError, match=rf"(^|[\s.,]){shown}\b"):
        call()
    assert ctx.calls == [], f"{name}: {ctx.calls} reached the context before the refusal"


@pytest.mark.parametrize("config", ("se_call_full", "nform_basis_se_call_vector", "everything_m"))
def test_what_the_contract_refuses_is_a_value_error_naming_the_argument(config):
    cfg = dict(CONFIGS[config], x0=True)
    good = named_tensors(cfg)
    with pointer_side() as ctx:
        for name, t in good.items():
            routes = routes_of(cfg) if name in CTOR_ARGS else [r for r in routes_of(cfg) if name in ROUTES[r][1]]
            for what, bad in bad_versions(t, {"b": 0, "xa": -2}.get(name, -1)):
                for route in routes:                                   # by the constructor, or at the latest by the call
                    refused(name, lambda: ROUTES[route][0](*case(cfg, lambda n, v: bad if n == name else v)), ctx)
        # z and p of another batch size than x; a per-profile xa and c_a of another batch size than the call's
        ov, a = case(cfg)
        for name in ("z", "p"):
            for rows in (NPROF - 1, NPROF + 1):
                b = types.SimpleNamespace(**dict(vars(a), **{name: getattr(a, name)[:1].expand(rows, -1).contiguous()}))
                for route in routes_of(cfg):
                    if name in ROUTES[route][1]:
                        refused(name, lambda: ROUTES[route][0](ov, b), ctx)
        grow = lambda t: torch.cat([t, t[-1:]], dim=0)    # noqa: E731
        for name in [n for n, on in (("xa", cfg.get("xa_per")), ("c_a", cfg.get("c_a_per"))) if on]:
            for route in routes_of(cfg):                               # (one per-profile prior contradicts the other first)
                refused("prior", lambda: ROUTES[route][0](*case(cfg, lambda n, v: grow(v) if n == name else v)), ctx)
        # NaN is no refusal: the kernels own it
        ov, a = case(cfg, lambda n, v: v.clone().index_fill_(0, torch.tensor([0]), float("nan")) if n == "x" else v)
        assert ROUTES["step"][0](ov, a)[1]["status"].tolist()[0] != 1 and ctx.calls


def test_the_instrument_refuses_what_it_cannot_hand_over():
    inst = Instrument(FRQ, ELEV, band=([-0.1, 0.1], [0.5, 0.5]))
    tb = torch.zeros((NPROF, inst.elev_q.size, inst.frq_q.size), dtype=torch.float64)
    k = torch.zeros(tuple(tb.shape) + (NLEV,), dtype=torch.float64)
    with pointer_side() as ctx:
        for what, bad in bad_versions(tb):
            with pytest.raises(ValueError, match="tb"):
                inst.apply(bad, [k])
        for what, bad in bad_versions(k):
            if what != "an extra dimension":                           # [1][nprof]... is one profile of more columns
                with pytest.raises(ValueError, match=r"k_blocks\[(0|1)\]"):
                    inst.apply(tb, [k, bad])
        assert ctx.calls == []
        inst.apply(every_other(tb), [permuted(k), offset(k)])
        assert ctx.calls == ["obs_create", "obs_apply_device"]


# ---- e: CPU tensors never reach the real library ---------------------------------------------------------------------------
def test_cpu_tensors_never_reach_the_native_context(monkeypatch):
    def forbidden(self, *args, **kwargs):
        raise AssertionError("a CPU tensor's pointer reached the native context")
    methods = {name: forbidden for name, v in vars(_native.Context).items() if callable(v) and not name.startswith("__")}
    native = object.__new__(type("ForbiddenContext", (_native.Context,), dict(methods, __del__=lambda self: None)))
    assert isinstance(native, _native.Context)
    monkeypatch.setattr(_native, "default_context", lambda device_id=0: native)
    for config in ("plain", "everything_m", "nform_basis_se_call_full"):
        cfg = CONFIGS[config]
        ov, a = case(cfg)
        for route in routes_of(cfg):
            with pytest.raises(ValueError, match="CUDA"):
                ROUTES[route][0](ov, a)
    inst = Instrument(FRQ, ELEV, band=([-0.1, 0.1], [0.5, 0.5]))
    with pytest.raises(ValueError, match="CUDA"):
        inst.apply(torch.zeros((NPROF, inst.elev_q.size, inst.frq_q.size), dtype=torch.float64))
