"""A pointer-faithful stand-in for ``_native.Context``, for the tests of the tensor contract of retrieval.py and
instrument.py (tests/test_tensor_contract_cpu.py) -- no GPU, no native library.

The other ``test_retrieval_*_cpu.py`` files replace the ``_native_*`` functions of retrieval.py themselves, so the code in
them -- which buffer goes to which argument, the flags, the row windows, the optional pointers -- never runs without a
GPU.  Here the real ``_native_*`` functions run, on top of a context that takes what the library takes: bare integers.

    log = track_pointers(monkeypatch)                 # every Tensor.data_ptr() handed out is recorded with its tensor
    ctx = PointerContext(log)
    monkeypatch.setattr(_native, "default_context", lambda device_id=0: ctx)

Every context method retrieval.py and instrument.py call has an entry in ``TABLE``: for each pointer argument its name, its
element type, the number of elements the C entry reads or writes there (from that entry's description in include/mwrt.h
and the call's integers and flags, never from the tensor), whether it may be NULL and whether it is written.  On a call
every non-NULL pointer must be the ``data_ptr()`` of a tensor recorded since the last call, of that dtype, contiguous, on
this context's device and with at least that many elements of storage behind the pointer -- otherwise ``ContractViolation``
names the method, the argument and what was found, and nothing is read.  Then the inputs are viewed as the flat arrays the
library would see, the outputs are computed by the tensor-level stand-ins of the ``*_cpu.py`` files (the NumPy references
oe_reference, oe_lm_reference, nform_reference, oe_char_reference, nform_char_reference, obs_reference, basis_reference
and whiten_reference) and written through the output pointers.  The same call through those stand-ins directly is
therefore the same NumPy code on the same numbers: any difference is the marshalling's.

The two K-matrix entries answer with the forward model of tests/test_retrieval_cpu.py (``Standins.forward``: linear,
optionally mildly curved) with one row of A per (elevation, frequency) node of whatever grid is asked for, plus a term in
z and p with unequal weights per level, so that neither can be swapped, shifted or permuted unnoticed."""
import ctypes
import inspect
import types
from collections import namedtuple

import numpy as np
import pytest
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native, retrieval
from test_retrieval_cpu import Standins as LinearModel
from test_retrieval_nform_char_cpu import NfCharStandins

F64, U8, I32 = torch.float64, torch.uint8, torch.int32
_CTYPE = {F64: ctypes.c_double, U8: ctypes.c_uint8, I32: ctypes.c_int32}


class ContractViolation(Exception):
    """A pointer reached the context that the library could not have read or written as its entry describes."""


# ---- the record of the pointers handed out ------------------------------------------------------------------------------
Record = namedtuple("Record", "tensor dtype shape stride extent device contiguous")


class PointerLog:
    def __init__(self):
        self.records = {}

    def add(self, ptr, t):
        behind = 0
        if t.device.type != "meta":
            behind = (t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()) // t.element_size()
        self.records[ptr] = Record(t, t.dtype, tuple(t.shape), tuple(t.stride()), behind, t.device, t.is_contiguous())

    def clear(self):
        self.records = {}


def track_pointers(monkeypatch):
    """Wraps ``torch.Tensor.data_ptr``: each pointer handed out is recorded with its tensor -- dtype, shape, strides, the
    elements of storage behind the pointer, device -- until the next context call clears the record."""
    log, real = PointerLog(), torch.Tensor.data_ptr

    def data_ptr(self):
        ptr = real(self)
        log.add(ptr, self)
        return ptr
    monkeypatch.setattr(torch.Tensor, "data_ptr", data_ptr)
    return log


# ---- the forward model of the K-matrix entries ---------------------------------------------------------------------------
class GridModel:
    """``test_retrieval_cpu.Standins.forward`` on any grid: A_b ``[nang * nf][nlev]`` is drawn per grid size; K = dF/dv."""

    def __init__(self, curve=0.0, seed=3):
        self.inner = object.__new__(LinearModel)             # its forward model alone: nothing is monkeypatched
        self.inner.curve, self.seed, self.calls = curve, seed, 0

    def k_matrix(self, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
        self.calls += 1
        nprof, nlev = t.shape
        rng = np.random.default_rng(self.seed + 1000 * frq.size * elev.size)
        self.inner.A = {b: torch.as_tensor(rng.uniform(0.2, 1.0, (elev.size * frq.size, nlev)) * s)
                        for b, s in (("t", 0.3), ("h", 8.0), ("liq", 20.0), ("ice", 5.0))}
        tb, lin = self.inner.forward(t, rh, denliq, denice)
        lev = torch.arange(1, nlev + 1, dtype=torch.float64)
        tb = tb + ((z * (0.01 * lev)).sum(dim=1) + (p * (1e-4 * lev.flip(0))).sum(dim=1))[:, None]
        slope = 1.0 + 2.0 * self.inner.curve * lin
        rows = {b: (slope[:, :, None] * self.inner.A[b][None]).reshape(nprof, elev.size, frq.size, nlev).contiguous()
                for b in want}
        return tb.reshape(nprof, elev.size, frq.size), torch.ones(nprof, dtype=torch.uint8), rows


class TensorStandins(NfCharStandins):
    """Every ``_native_*`` seam of retrieval.py replaced at tensor level, as the ``*_cpu.py`` files do: their stand-ins, with
    ``GridModel`` behind the two K-matrix seams (a different one behind the ray seam).  With ``monkeypatch=None`` nothing
    stays patched: the object then only computes, for ``PointerContext``."""

    def __init__(self, monkeypatch=None, curve=2e-3):
        own = pytest.MonkeyPatch() if monkeypatch is None else None
        super().__init__(own or monkeypatch)
        self.model, self.ray_model = GridModel(curve, seed=3), GridModel(curve, seed=11)
        (own or monkeypatch).setattr(retrieval, "_native_k_matrix", self.model.k_matrix)
        (own or monkeypatch).setattr(retrieval, "_native_k_matrix_ray", self.ray_model.k_matrix)
        if own is not None:
            own.undo()


# ---- the table: what each entry reads and writes through its pointers -----------------------------------------------------
Arg = namedtuple("Arg", "name dtype count optional out each")
Entry = namedtuple("Entry", "args flags")


def arg(name, dtype, count, optional=False, out=False, each=False):
    """``count(c)``: elements behind the pointer, from the call's arguments ``c``; ``each``: a sequence of pointers."""
    return Arg(name, dtype, count, optional, out, each)


_lev = lambda c: c.nprof * c.nlev                      # noqa: E731  [nprof][nlev]
_node = lambda c: c.nprof * c.nang * c.nf              # noqa: E731  [nprof][nang][nf]
_row = lambda c: c.nprof * c.nang * c.nf * c.nlev      # noqa: E731  [nprof][nang][nf][nlev]
_k = lambda c: c.nprof * c.m * c.nlev                  # noqa: E731  [nprof][m][nlev]
_x = lambda c: c.nprof * c.nblk * c.nlev               # noqa: E731  [nprof][nblk][nlev]
_xa = lambda c: (c.nprof if c.xa_per_profile else 1) * c.nblk * c.nlev    # noqa: E731
_nn = lambda c: c.n * c.n                              # noqa: E731  [n][n]
_se = lambda c: c.m * c.m if c.se_full else c.m        # noqa: E731  [m] or [m][m]
_sev = lambda c: c.nprof * c.m if c.se_per_profile else c.m               # noqa: E731  [m] or [nprof][m]
_pm = lambda c: c.nprof * c.m                          # noqa: E731  [nprof][m]
_p = lambda c: c.nprof                                 # noqa: E731  [nprof]
_tri_m = lambda c: c.nprof * (c.m * (c.m + 1) // 2)    # noqa: E731  [nprof][m (m + 1) / 2]
_tri_n = lambda c: c.nprof * (c.n * (c.n + 1) // 2)    # noqa: E731  [nprof][n (n + 1) / 2]
_pnn = lambda c: c.nprof * c.n * c.n                   # noqa: E731  [nprof][n][n]
_pmn = lambda c: c.nprof * c.m * c.n                   # noqa: E731  [nprof][m][n]
_win = lambda c: c.nprof * (c.row_count or c.n) * c.n  # noqa: E731  [nprof][rows][n]

_K_MATRIX = Entry([
    arg("d_z", F64, _lev), arg("d_p", F64, _lev), arg("d_t", F64, _lev), arg("d_rh", F64, _lev),
    arg("d_tb", F64, _node, out=True), arg("d_dtb_dt", F64, _row, out=True), arg("d_dtb_dh", F64, _row, out=True),
    arg("d_valid", U8, _p, out=True), arg("d_denliq", F64, _lev, optional=True), arg("d_denice", F64, _lev, optional=True),
    arg("d_dtb_dliq", F64, _row, optional=True, out=True), arg("d_dtb_dice", F64, _row, optional=True, out=True)], ())
_STEP_IN = [arg("d_k", F64, _k, each=True), arg("d_x", F64, _x), arg("d_xa", F64, _xa), arg("d_sa", F64, _nn),
            arg("d_se", F64, _se), arg("d_y", F64, _pm), arg("d_fx", F64, _pm)]
_LM_LIN = lambda out: [arg("d_g0", F64, _tri_m, out=out), arg("d_r", F64, _pm, out=out), arg("d_kdx", F64, _pm, out=out),    # noqa: E731
                       arg("d_keep", U8, _pm, out=out), arg("d_lin_status", U8, _p, out=out)]
_ACTIVE = arg("d_active", U8, _p, optional=True)

TABLE = {
    "tb_jacobian_batch_vars_device": _K_MATRIX,
    "tb_jacobian_batch_ray_device": _K_MATRIX,
    "oe_step_device": Entry(_STEP_IN + [
        arg("d_x_new", F64, _x, out=True), arg("d_status", U8, _p, out=True), arg("d_chi2", F64, _p, optional=True, out=True),
        arg("d_dfs", F64, _p, optional=True, out=True), arg("d_post_var", F64, _x, optional=True, out=True),
        arg("d_nobs", I32, _p, optional=True, out=True)], ("xa_per_profile", "se_full")),
    "oe_lm_prepare_device": Entry(_STEP_IN + _LM_LIN(True) + [_ACTIVE], ("xa_per_profile", "se_full")),
    "oe_lm_solve_device": Entry(_STEP_IN[:5] + [arg("d_gamma", F64, _p)] + _LM_LIN(False) + [
        arg("d_x_new", F64, _x, out=True), arg("d_status", U8, _p, out=True), _ACTIVE], ("xa_per_profile", "se_full")),
    "oe_cost_device": Entry([
        arg("d_x", F64, _x), arg("d_xa", F64, _xa), arg("d_se", F64, _se), arg("d_y", F64, _pm), arg("d_fx", F64, _pm),
        arg("d_keep", U8, _pm), arg("d_sa_inv", F64, _nn), arg("d_cost", F64, _p, out=True), _ACTIVE],
        ("xa_per_profile", "se_full")),
    "oe_nform_prepare_device": Entry([
        arg("d_k", F64, _k, each=True), arg("d_x", F64, _x), arg("d_xa", F64, _xa), arg("d_se", F64, _sev),
        arg("d_y", F64, _pm), arg("d_fx", F64, _pm), arg("d_h", F64, _tri_n, out=True), arg("d_g", F64, lambda c: c.nprof * c.n, out=True),
        arg("d_rwr", F64, _p, out=True), arg("d_keep", U8, _pm, out=True), arg("d_nobs", I32, _p, out=True),
        arg("d_lin_status", U8, _p, out=True), _ACTIVE], ("xa_per_profile", "se_per_profile")),
    "oe_nform_solve_device": Entry([
        arg("d_x", F64, _x), arg("d_xa", F64, _xa), arg("d_sa_inv", F64, _nn), arg("d_h", F64, _tri_n),
        arg("d_g", F64, lambda c: c.nprof * c.n), arg("d_rwr", F64, _p), arg("d_lin_status", U8, _p),
        arg("d_x_new", F64, _x, out=True), arg("d_status", U8, _p, out=True), arg("d_gamma", F64, _p, optional=True),
        arg("d_chi2", F64, _p, optional=True, out=True), arg("d_dfs", F64, _p, optional=True, out=True),
        arg("d_post_var", F64, _x, optional=True, out=True), arg("d_post_cov", F64, _pnn, optional=True, out=True), _ACTIVE],
        ("xa_per_profile",)),
    "oe_nform_cost_device": Entry([
        arg("d_x", F64, _x), arg("d_xa", F64, _xa), arg("d_sa_inv", F64, _nn), arg("d_se", F64, _sev), arg("d_y", F64, _pm),
        arg("d_fx", F64, _pm), arg("d_keep", U8, _pm), arg("d_cost", F64, _p, out=True), _ACTIVE],
        ("xa_per_profile", "se_per_profile")),
    "oe_nform_char_device": Entry([
        arg("d_sa_inv", F64, _nn), arg("d_h", F64, _tri_n), arg("d_lin_status", U8, _p), arg("d_status", U8, _p, out=True),
        arg("d_post_cov", F64, _pnn, optional=True, out=True), arg("d_avk", F64, _win, optional=True, out=True),
        arg("d_avk_diag", F64, _x, optional=True, out=True), arg("d_dfs_block", F64, lambda c: c.nprof * c.nblk, optional=True, out=True),
        arg("d_noise_var", F64, _x, optional=True, out=True), arg("d_smooth_var", F64, _x, optional=True, out=True)],
        ("row_count",)),
    "oe_nform_gain_device": Entry([
        arg("d_k", F64, _k, each=True), arg("d_se", F64, _sev), arg("d_keep", U8, _pm), arg("d_post_cov", F64, _pnn),
        arg("d_status", U8, _p), arg("d_gain", F64, _pmn, out=True)], ("se_per_profile",)),
    "oe_gain_device": Entry(_STEP_IN + [
        arg("d_status", U8, _p, out=True), arg("d_gain", F64, _pmn, optional=True, out=True),
        arg("d_ksa", F64, _pmn, optional=True, out=True), arg("d_keep", U8, _pm, optional=True, out=True),
        arg("d_avk_diag", F64, _x, optional=True, out=True), arg("d_dfs_block", F64, lambda c: c.nprof * c.nblk, optional=True, out=True),
        arg("d_noise_var", F64, _x, optional=True, out=True), arg("d_smooth_var", F64, _x, optional=True, out=True),
        arg("d_nobs", I32, _p, optional=True, out=True)], ("xa_per_profile", "se_full")),
    # the product reads d_k for the averaging kernel and d_ksa, d_sa for the posterior covariance: 0 elements otherwise
    "oe_product_device": Entry([
        arg("d_gain", F64, _pmn), arg("d_keep", U8, _pm), arg("d_out", F64, _win, out=True),
        arg("d_k", F64, lambda c: _k(c) if c.product == _native.OE_PRODUCT_AVK else 0, each=True),
        arg("d_ksa", F64, lambda c: _pmn(c) if c.product == _native.OE_PRODUCT_POST_COV else 0, optional=True),
        arg("d_sa", F64, lambda c: _nn(c) if c.product == _native.OE_PRODUCT_POST_COV else 0, optional=True)],
        ("product", "row_count")),
    "obs_create": Entry([], ()),
    "obs_destroy": Entry([], ()),
    "obs_apply_device": Entry([
        arg("d_tb_in", F64, lambda c: c.nprof * c.m_in, optional=True), arg("d_tb_out", F64, lambda c: c.nprof * c.m_out, optional=True, out=True),
        arg("d_k_in", F64, lambda c: c.nprof * c.m_in * c.nlev, each=True),
        arg("d_k_out", F64, lambda c: c.nprof * c.m_out * c.nlev, out=True, each=True)], ()),
    "basis_create": Entry([], ()),
    "basis_destroy": Entry([], ()),
    "basis_project_device": Entry([
        arg("d_k_in", F64, lambda c: c.nprof * c.m * c.nlev, each=True), arg("d_k_out", F64, lambda c: c.nprof * c.m * c.r, out=True)], ()),
    "basis_expand_device": Entry([
        arg("d_c", F64, lambda c: c.nprof * c.r), arg("d_x_ref", F64, lambda c: (c.nprof if c.x_ref_per_profile else 1) * c.n),
        arg("d_x", F64, lambda c: c.nprof * c.n, out=True)], ("x_ref_per_profile",)),
    "obs_whiten_device": Entry([
        arg("d_se", F64, lambda c: c.nprof * (c.m * c.m if c.se_full else c.m)), arg("d_y", F64, _pm), arg("d_fx", F64, _pm),
        arg("d_k_in", F64, _k, each=True), arg("d_l", F64, _tri_m, out=True), arg("d_keep", U8, _pm, out=True),
        arg("d_status", U8, _p, out=True), arg("d_y_out", F64, _pm, optional=True, out=True),
        arg("d_fx_out", F64, _pm, optional=True, out=True), arg("d_k_out", F64, _k, out=True, each=True)], ("se_full",)),
    "obs_whiten_apply_device": Entry([
        arg("d_l", F64, _tri_m), arg("d_keep", U8, _pm), arg("d_y", F64, _pm, optional=True),
        arg("d_y_out", F64, _pm, optional=True, out=True), arg("d_k_in", F64, _k, each=True),
        arg("d_k_out", F64, _k, out=True, each=True)], ("mode",)),
}


# ---- the context -------------------------------------------------------------------------------------------------------
class PointerContext:
    """See the module docstring.  ``calls`` lists the methods called; ``seen[method][argument]`` collects "null" / "set" and
    ``flags[method][flag]`` the values each flag took (``row_count`` as ``> 0``); ``last[method]`` keeps the latest call for
    ``replay``."""
    _handle = True                                            # ``native_handle`` asks whether the context is still open

    def __init__(self, log, device="cpu", curve=2e-3):
        self.log, self.device = log, torch.device(device)
        self.st = TensorStandins(None, curve=curve)
        self.calls, self.last = [], {}
        self.seen = {m: {a.name: set() for a in e.args} for m, e in TABLE.items()}
        self.flags = {m: {f: set() for f in e.flags} for m, e in TABLE.items()}

    # -- handles: host arrays, no device pointers ------------------------------------------------------------------------
    def obs_create(self, m_in, m_out, row_ptr, col, w):
        self.calls.append("obs_create")
        return types.SimpleNamespace(m_in=int(m_in), m_out=int(m_out), row_ptr=np.array(row_ptr, dtype=np.int32),
                                     col=np.array(col, dtype=np.int32), w=np.array(w, dtype=np.float64), alive=True,
                                     elev=np.zeros(1), frq=np.zeros(int(m_out)))      # obs_reference's output: [1][m_out]

    def basis_create(self, nblk, nlev, b):
        self.calls.append("basis_create")
        b = np.array(b, dtype=np.float64)
        if b.ndim != 2 or b.shape[0] != int(nblk) * int(nlev):
            raise ContractViolation(f"basis_create: expected b [{int(nblk) * int(nlev)}][r], got {b.shape}")
        return types.SimpleNamespace(nblk=int(nblk), nlev=int(nlev), n=b.shape[0], r=b.shape[1], b=torch.as_tensor(b), alive=True)

    def obs_destroy(self, handle):
        self.calls.append("obs_destroy")
        handle.alive = False

    def basis_destroy(self, handle):
        self.calls.append("basis_destroy")
        handle.alive = False

    # -- the entries that take pointers ----------------------------------------------------------------------------------
    def _call(self, method, args, kwargs, remember=True):
        entry = TABLE[method]
        try:
            bound = inspect.signature(getattr(_native.Context, method)).bind(self, *args, **kwargs)
            bound.apply_defaults()
            c = types.SimpleNamespace(**bound.arguments)
            self._derive(method, c)
            known = {a.name for a in entry.args}
            views, todo = {}, []
            for name, v in bound.arguments.items():
                if name.startswith("d_") and name not in known and v is not None and len(np.atleast_1d(v)):
                    raise ContractViolation(f"{method}: {name} is a pointer argument without an entry in TABLE")
            for a in entry.args:
                given = getattr(c, a.name)
                ptrs = list(given) if a.each else [given]
                self.seen[method][a.name].add("set" if ptrs and all(p is not None for p in ptrs) else "null")
                count = int(a.count(c))
                for i, ptr in enumerate(ptrs):
                    label = f"{a.name}[{i}]" if a.each else a.name
                    if ptr is None:
                        if not a.optional and count:
                            raise ContractViolation(f"{method}: {label} is NULL but the entry requires it")
                    elif count:
                        todo.append((a, label, self._resolved(method, label, ptr, a.dtype, count), count))
                views[a.name] = [] if a.each else None
            for a, label, ptr, count in todo:                    # every pointer has passed: now, and only now, read
                flat = torch.from_numpy(np.ctypeslib.as_array((_CTYPE[a.dtype] * count).from_address(ptr)))
                if a.each:
                    views[a.name].append(flat)
                else:
                    views[a.name] = flat
            for f in entry.flags:
                v = getattr(c, f)
                self.flags[method][f].add(bool(v) if f in ("row_count", "xa_per_profile", "se_full", "se_per_profile",
                                                              "x_ref_per_profile") else int(v))
            if remember:
                self.last[method] = (args, kwargs, dict(self.log.records))
            self.calls.append(method)
            getattr(self, "_do_" + method)(c, views)
        finally:
            self.log.clear()

    def _resolved(self, method, label, ptr, dtype, count):
        if not isinstance(ptr, int):
            raise ContractViolation(f"{method}: {label} is not an integer address but {type(ptr).__name__}")
        rec = self.log.records.get(ptr)
        if rec is None:
            raise ContractViolation(f"{method}: {label} = {ptr:#x} is not the data_ptr() of a tensor handed out for this call")
        what = f"a {rec.dtype} tensor {rec.shape} with strides {rec.stride} on {rec.device}"
        if rec.dtype != dtype:
            raise ContractViolation(f"{method}: {label} is read as {count} elements of {dtype}, got {what}")
        if rec.device != self.device:
            raise ContractViolation(f"{method}: {label} must be on {self.device}, got {what}")
        if not rec.contiguous:
            raise ContractViolation(f"{method}: {label} is read as {count} contiguous elements, got {what}")
        if rec.extent < count:
            raise ContractViolation(f"{method}: {label} is read as {count} elements but only {rec.extent} lie behind the pointer of {what}")
        return ptr

    @staticmethod
    def _derive(method, c):
        """The sizes the counts are written in, from the call's integers alone."""
        if hasattr(c, "frq"):
            c.nf, c.nang = np.asarray(c.frq).size, np.asarray(c.elev).size
        if hasattr(c, "handle"):
            if not c.handle.alive:
                raise ContractViolation(f"{method}: the handle was destroyed")
            for key in ("m_in", "m_out", "r", "n"):
                if hasattr(c.handle, key):
                    setattr(c, key, getattr(c.handle, key))
            if method == "basis_project_device":
                c.nlev = c.handle.nlev
                if len(list(c.d_k_in)) != c.handle.nblk:
                    raise ContractViolation(f"{method}: {len(list(c.d_k_in))} blocks for a basis of {c.handle.nblk}")
        if getattr(c, "nblk", None) is None:
            for name in ("d_k", "d_k_in"):
                if hasattr(c, name):
                    c.nblk = len(list(getattr(c, name)))
        if hasattr(c, "nlev") and getattr(c, "nblk", None) is not None and not hasattr(c, "n"):
            c.n = c.nblk * c.nlev
        if hasattr(c, "row_count") and (c.row_begin < 0 or c.row_count < 0 or c.row_begin + c.row_count > c.n
                                        or (c.row_count == 0 and c.row_begin != 0)):
            raise ContractViolation(f"{method}: rows {c.row_begin} + {c.row_count} outside 0 .. {c.n - 1}")

    def replay(self, method, **changes):
        """The latest call of ``method`` again, with some keyword arguments replaced (e.g. an optional pointer by None)."""
        args, kwargs, records = self.last[method]
        names = list(inspect.signature(getattr(_native.Context, method)).parameters)[1:]
        kwargs = dict(zip(names, args), **kwargs)
        kwargs.update(changes)
        self.log.records = dict(records)
        self._call(method, (), kwargs, remember=False)

    @staticmethod
    def _store(views, out, **names):
        for ptr_name, key in names.items():
            if views[ptr_name] is not None:
                views[ptr_name][:] = torch.as_tensor(out[key]).reshape(-1)

    @staticmethod
    def _step_inputs(c, v):
        xa_shape = (c.nprof, c.nblk, c.nlev) if c.xa_per_profile else (c.nblk, c.nlev)
        out = dict(x=v["d_x"].reshape(c.nprof, c.nblk, c.nlev), xa=v["d_xa"].reshape(xa_shape))
        if v.get("d_k"):
            out["k"] = [k.reshape(c.nprof, c.m, c.nlev) for k in v["d_k"]]
        if v.get("d_sa") is not None:
            out["sa"] = v["d_sa"].reshape(c.n, c.n)
        if v.get("d_sa_inv") is not None:
            out["sa_inv"] = v["d_sa_inv"].reshape(c.n, c.n)
        if v.get("d_se") is not None:
            full = getattr(c, "se_full", False)
            per = getattr(c, "se_per_profile", False)
            out["se"] = v["d_se"].reshape((c.m, c.m) if full else (c.nprof, c.m) if per else (c.m,))
        for key in ("y", "fx", "keep", "r", "kdx"):
            if v.get("d_" + key) is not None:
                out[key] = v["d_" + key].reshape(c.nprof, c.m)
        return types.SimpleNamespace(**out)

    @staticmethod
    def _active(c, v):
        return torch.ones(c.nprof, dtype=torch.uint8) if v["d_active"] is None else v["d_active"]

    def _k_matrix(self, c, v, seam):
        sh = (c.nprof, c.nlev)
        opt = lambda key: None if v[key] is None else v[key].reshape(sh)   # noqa: E731
        want = ("t", "h") + (("liq",) if v["d_dtb_dliq"] is not None else ()) + (("ice",) if v["d_dtb_dice"] is not None else ())
        frq, elev = np.asarray(c.frq, dtype=np.float64).ravel(), np.asarray(c.elev, dtype=np.float64).ravel()
        tb, valid, rows = seam(c.model, v["d_z"].reshape(sh), v["d_p"].reshape(sh), v["d_t"].reshape(sh), v["d_rh"].reshape(sh),
                               opt("d_denliq"), opt("d_denice"), frq, elev, c.variables, want, None)
        self._store(v, dict(rows, tb=tb, valid=valid), d_tb="tb", d_valid="valid", d_dtb_dt="t", d_dtb_dh="h",
                    **{"d_dtb_d" + b: b for b in want[2:]})

    def _do_tb_jacobian_batch_vars_device(self, c, v):
        self._k_matrix(c, v, self.st.model.k_matrix)

    def _do_tb_jacobian_batch_ray_device(self, c, v):
        self._k_matrix(c, v, self.st.ray_model.k_matrix)

    def _do_oe_step_device(self, c, v):
        i = self._step_inputs(c, v)
        out = self.st.oe_step(i.k, i.x, i.xa, i.sa, i.se, i.y, i.fx, v["d_post_var"] is not None, None)
        self._store(v, out, d_x_new="x_new", d_status="status", d_chi2="chi2", d_dfs="dfs", d_nobs="nobs",
                    **({} if out["post_var"] is None else {"d_post_var": "post_var"}))

    def _lm_lin(self, c, v):
        return dict(g0=v["d_g0"].reshape(c.nprof, -1), r=v["d_r"].reshape(c.nprof, c.m), kdx=v["d_kdx"].reshape(c.nprof, c.m),
                    keep=v["d_keep"].reshape(c.nprof, c.m), lin_status=v["d_lin_status"])

    def _do_oe_lm_prepare_device(self, c, v):
        i = self._step_inputs(c, v)
        self.st.oe_lm_prepare(i.k, i.x, i.xa, i.sa, i.se, i.y, i.fx, self._lm_lin(c, v), self._active(c, v), None)

    def _do_oe_lm_solve_device(self, c, v):
        i = self._step_inputs(c, v)
        out = dict(x_new=v["d_x_new"].reshape(c.nprof, c.nblk, c.nlev), status=v["d_status"])
        self.st.oe_lm_solve(i.k, i.x, i.xa, i.sa, i.se, v["d_gamma"], self._lm_lin(c, v), out, self._active(c, v), None)

    def _do_oe_cost_device(self, c, v):
        i = self._step_inputs(c, v)
        self.st.oe_cost(i.x, i.xa, i.se, i.y, i.fx, i.keep, i.sa_inv, v["d_cost"], self._active(c, v), None)

    def _nform_lin(self, c, v):
        names = ("h", "g", "rwr", "keep", "nobs", "lin_status")
        shape = dict(h=(c.nprof, -1), g=(c.nprof, c.n), keep=(c.nprof, c.m))
        return {k: v["d_" + k].reshape(shape.get(k, (c.nprof,))) for k in names if v.get("d_" + k) is not None}

    def _do_oe_nform_prepare_device(self, c, v):
        i = self._step_inputs(c, v)
        self.st.oe_nform_prepare(i.k, i.x, i.xa, i.se, i.y, i.fx, self._nform_lin(c, v), v["d_active"], None)

    def _do_oe_nform_solve_device(self, c, v):
        i = self._step_inputs(c, v)
        shape = dict(x_new=(c.nprof, c.nblk, c.nlev), post_var=(c.nprof, c.nblk, c.nlev), post_cov=(c.nprof, c.n, c.n))
        out = {k: v["d_" + k].reshape(shape.get(k, (c.nprof,))) for k in ("x_new", "status", "chi2", "dfs", "post_var", "post_cov")
               if v["d_" + k] is not None}
        if v["d_gamma"] is not None and set(out) - {"x_new", "status"}:
            raise ContractViolation("oe_nform_solve_device: chi2, dfs, post_var and post_cov are defined without d_gamma only")
        self.st.oe_nform_solve(i.x, i.xa, i.sa_inv, self._nform_lin(c, v), v["d_gamma"], out, v["d_active"], None)

    def _do_oe_nform_cost_device(self, c, v):
        i = self._step_inputs(c, v)
        self.st.oe_nform_cost(i.x, i.xa, i.sa_inv, i.se, i.y, i.fx, i.keep, v["d_cost"], v["d_active"], None)

    def _do_oe_nform_char_device(self, c, v):
        x = (c.nprof, c.nblk, c.nlev)
        shape = dict(status=(c.nprof,), post_cov=(c.nprof, c.n, c.n), avk=(c.nprof, c.row_count or c.n, c.n), avk_diag=x,
                     dfs_block=(c.nprof, c.nblk), noise_var=x, smooth_var=x)
        out = {k: v["d_" + k].reshape(s) for k, s in shape.items() if v["d_" + k] is not None}
        if len(out) < 2:
            raise ContractViolation("oe_nform_char_device: at least one optional output must be given")
        self.st.oe_nform_char(v["d_sa_inv"].reshape(c.n, c.n), self._nform_lin(c, v), c.nblk, out, (c.row_begin, c.row_count), None)

    def _do_oe_nform_gain_device(self, c, v):
        se = v["d_se"].reshape((c.nprof, c.m) if c.se_per_profile else (c.m,))
        gain = self.st.oe_nform_gain([k.reshape(c.nprof, c.m, c.nlev) for k in v["d_k"]], se, v["d_keep"].reshape(c.nprof, c.m),
                                     v["d_post_cov"].reshape(c.nprof, c.n, c.n), v["d_status"], None)
        self._store(v, dict(gain=gain), d_gain="gain")

    def _do_oe_gain_device(self, c, v):
        i = self._step_inputs(c, v)
        names = ("status", "gain", "ksa", "keep", "avk_diag", "dfs_block", "noise_var", "smooth_var", "nobs")
        if all(v["d_" + k] is None for k in names[1:]):
            raise ContractViolation("oe_gain_device: at least one optional output must be given")
        self._store(v, self.st.oe_gain(i.k, i.x, i.xa, i.sa, i.se, i.y, i.fx, None), **{"d_" + k: k for k in names})

    def _do_oe_product_device(self, c, v):
        avk = c.product == _native.OE_PRODUCT_AVK
        if c.product not in (_native.OE_PRODUCT_AVK, _native.OE_PRODUCT_POST_COV) or (not avk and (v["d_ksa"] is None or v["d_sa"] is None)):
            raise ContractViolation(f"oe_product_device: product {c.product} without what it reads")
        k = [b.reshape(c.nprof, c.m, c.nlev) for b in v["d_k"]] if avk else [None] * c.nblk
        out = self.st.oe_product("avk" if avk else "post_cov", v["d_gain"].reshape(c.nprof, c.m, c.n), v["d_keep"].reshape(c.nprof, c.m),
                                 k, None if avk else v["d_ksa"].reshape(c.nprof, c.m, c.n), None if avk else v["d_sa"].reshape(c.n, c.n),
                                 (c.row_begin, c.row_count), None)
        self._store(v, dict(out=out), d_out="out")

    def _do_obs_apply_device(self, c, v):
        if (v["d_tb_in"] is None) != (v["d_tb_out"] is None) or len(v["d_k_in"]) != len(v["d_k_out"]):
            raise ContractViolation("obs_apply_device: inputs and outputs come in pairs")
        tb = None if v["d_tb_in"] is None else v["d_tb_in"].reshape(c.nprof, c.m_in)
        k = [b.reshape(c.nprof, c.m_in, c.nlev) for b in v["d_k_in"]]
        tb_out, k_out = self.st.obs_apply(c.handle, tb, k or None, None)
        self._store(v, dict(tb=tb_out), d_tb_out="tb")
        for dst, src in zip(v["d_k_out"], k_out or []):
            dst[:] = src.reshape(-1)

    def _do_basis_project_device(self, c, v):
        out = self.st.basis_project(c.handle, [k.reshape(c.nprof, c.m, c.nlev) for k in v["d_k_in"]], None)
        self._store(v, dict(out=out), d_k_out="out")

    def _do_basis_expand_device(self, c, v):
        h = c.handle
        x_ref = v["d_x_ref"].reshape((c.nprof, h.nblk, h.nlev) if c.x_ref_per_profile else (h.nblk, h.nlev))
        self._store(v, dict(x=self.st.basis_expand(h, v["d_c"].reshape(c.nprof, h.r), x_ref, None)), d_x="x")

    def _do_obs_whiten_device(self, c, v):
        if len(v["d_k_in"]) != len(v["d_k_out"]):
            raise ContractViolation("obs_whiten_device: one output block per input block")
        se = v["d_se"].reshape((c.nprof, c.m, c.m) if c.se_full else (c.nprof, c.m))
        out = self.st.obs_whiten([k.reshape(c.nprof, c.m, c.nlev) for k in v["d_k_in"]], se, v["d_y"].reshape(c.nprof, c.m),
                                 v["d_fx"].reshape(c.nprof, c.m), None)
        self._store(v, out, d_l="l", d_keep="keep", d_status="status", d_y_out="y", d_fx_out="fx")
        for dst, src in zip(v["d_k_out"], out["k"]):
            dst[:] = src.reshape(-1)

    def _do_obs_whiten_apply_device(self, c, v):
        if (v["d_y"] is None) != (v["d_y_out"] is None) or len(v["d_k_in"]) != len(v["d_k_out"]) or len(v["d_k_in"]) > 1:
            raise ContractViolation("obs_whiten_apply_device: inputs and outputs come in pairs, one block at the most")
        vec = None if v["d_y"] is None else v["d_y"].reshape(c.nprof, c.m)
        block = v["d_k_in"][0].reshape(c.nprof, c.m, c.nlev) if v["d_k_in"] else None
        v_out, b_out = self.st.obs_whiten_apply(v["d_l"].reshape(c.nprof, -1), v["d_keep"].reshape(c.nprof, c.m), c.mode, vec, block, None)
        self._store(v, dict(y=v_out), d_y_out="y")
        if block is not None:
            v["d_k_out"][0][:] = b_out.reshape(-1)


def _entry(method):
    def call(self, *args, **kwargs):
        return self._call(method, args, kwargs)
    call.__name__ = method
    return call


for _method, _e in TABLE.items():
    if _e.args:
        setattr(PointerContext, _method, _entry(_method))
