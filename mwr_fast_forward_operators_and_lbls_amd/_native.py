"""ctypes binding of libmwrt.so (include/mwrt.h).  No fallback: if the HIP library or a GPU is
missing every compute entry point raises -- the product never routes through a CPU path."""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Dict, Optional

import numpy as np

from .spectroscopy import ModelTables, MwrtModelDesc, get_model

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmwrt.so")

c_double_p = ctypes.POINTER(ctypes.c_double)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)


class MwrtError(RuntimeError):
    """A non-zero mwrt_status came back across the C ABI."""

    def __init__(self, code: int, where: str, text: str):
        super().__init__(f"{where} failed with status {code}: {text}")
        self.code = code


class NativeLibraryMissing(ImportError):
    pass


class MwrtTbExtras(ctypes.Structure):
    _fields_ = [("tbatm", ctypes.c_void_p), ("tmr", ctypes.c_void_p), ("tauwet", ctypes.c_void_p),
                ("taudry", ctypes.c_void_p), ("taulay", ctypes.c_void_p), ("tauliq", ctypes.c_void_p),
                ("tauice", ctypes.c_void_p)]


class MwrtTbOptions(ctypes.Structure):
    """include/mwrt.h mwrt_tb_options: the opt-in physics (cloud liquid / ice, ray tracing)."""
    _fields_ = [("denliq", ctypes.c_void_p), ("denice", ctypes.c_void_p), ("ray_tracing", ctypes.c_int32),
                ("reserved0", ctypes.c_int32), ("o3n", ctypes.c_void_p)]


class JacVariables(ctypes.Structure):
    """include/mwrt.h mwrt_jac_variables: the variables the device K-matrix is returned in."""
    _fields_ = [("humidity", ctypes.c_int32), ("cloud", ctypes.c_int32), ("heights", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    HUMIDITY = {"e": 0, "rh": 1, "ppmv": 2}
    CLOUD = {"density": 0, "kg/kg": 1}
    HEIGHTS = {"fixed": 0, "hydrostatic": 1}

    @classmethod
    def of(cls, humidity="e", cloud="density", heights="fixed", reserved=0):
        """Names (or the ABI's integers, passed through unchecked: the library refuses what is out of range)."""
        pick = lambda table, x: table[x] if isinstance(x, str) else int(x)   # noqa: E731
        return cls(pick(cls.HUMIDITY, humidity), pick(cls.CLOUD, cloud), pick(cls.HEIGHTS, heights), int(reserved))


class MwrtOeStep(ctypes.Structure):
    """include/mwrt.h mwrt_oe_step: the record of one optimal-estimation step (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("xa_per_profile", ctypes.c_int32),
                ("se_full", ctypes.c_int32), ("reserved", ctypes.c_int32), ("d_k", ctypes.c_void_p * 4),
                ("d_x", ctypes.c_void_p), ("d_xa", ctypes.c_void_p), ("d_sa", ctypes.c_void_p), ("d_se", ctypes.c_void_p),
                ("d_y", ctypes.c_void_p), ("d_fx", ctypes.c_void_p), ("d_x_new", ctypes.c_void_p),
                ("d_status", ctypes.c_void_p), ("d_chi2", ctypes.c_void_p), ("d_dfs", ctypes.c_void_p),
                ("d_post_var", ctypes.c_void_p), ("d_nobs", ctypes.c_void_p)]


class MwrtOeLm(ctypes.Structure):
    """include/mwrt.h mwrt_oe_lm: the record of the Levenberg-Marquardt split of the step (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("xa_per_profile", ctypes.c_int32),
                ("se_full", ctypes.c_int32), ("reserved", ctypes.c_int32), ("d_k", ctypes.c_void_p * 4)] + [
        (name, ctypes.c_void_p) for name in (
            "d_x", "d_xa", "d_sa", "d_se", "d_y", "d_fx", "d_gamma", "d_g0", "d_r", "d_kdx", "d_keep", "d_lin_status",
            "d_active", "d_sa_inv", "d_cost", "d_cost_obs", "d_cost_prior", "d_x_new", "d_status", "d_chi2", "d_nobs")]


class MwrtOeNform(ctypes.Structure):
    """include/mwrt.h mwrt_oe_nform: the record of the n-form of the step (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("xa_per_profile", ctypes.c_int32),
                ("se_per_profile", ctypes.c_int32), ("reserved", ctypes.c_int32), ("d_k", ctypes.c_void_p * 4)] + [
        (name, ctypes.c_void_p) for name in (
            "d_x", "d_xa", "d_sa_inv", "d_se", "d_y", "d_fx", "d_gamma", "d_active", "d_h", "d_g", "d_rwr", "d_keep",
            "d_nobs", "d_lin_status", "d_x_new", "d_status", "d_chi2", "d_dfs", "d_post_var", "d_post_cov", "d_cost",
            "d_cost_obs", "d_cost_prior")]


class MwrtOeNformChar(ctypes.Structure):
    """include/mwrt.h mwrt_oe_nform_char: the record of the n-form's characterisation and gain entries (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("se_per_profile", ctypes.c_int32),
                ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("d_k", ctypes.c_void_p * 4)] + [
        (name, ctypes.c_void_p) for name in (
            "d_sa_inv", "d_se", "d_h", "d_lin_status", "d_keep", "d_active", "d_status", "d_post_cov", "d_avk", "d_avk_diag",
            "d_noise_var", "d_smooth_var", "d_dfs_block", "d_gain")]


class MwrtOeSelect(ctypes.Structure):
    """include/mwrt.h mwrt_oe_select: the record of the observation selection (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("se_per_profile", ctypes.c_int32),
                ("s0_per_profile", ctypes.c_int32), ("nsel", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("d_k", ctypes.c_void_p * 4)] + [
        (name, ctypes.c_void_p) for name in (
            "d_s0", "d_se", "d_sa_inv", "d_keep", "d_candidate", "d_active", "d_order", "d_q_pick", "d_rank", "d_q", "d_count",
            "d_status", "d_dfs_gain", "d_post_cov", "d_post_var")]


class MwrtOeChar(ctypes.Structure):
    """include/mwrt.h mwrt_oe_char: the record of the gain and product entries (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("xa_per_profile", ctypes.c_int32),
                ("se_full", ctypes.c_int32), ("reserved", ctypes.c_int32), ("d_k", ctypes.c_void_p * 4)] + [
        (name, ctypes.c_void_p) for name in (
            "d_x", "d_xa", "d_sa", "d_se", "d_y", "d_fx", "d_status", "d_gain", "d_ksa", "d_keep", "d_avk_diag",
            "d_dfs_block", "d_noise_var", "d_smooth_var", "d_nobs")] + [
        (name, ctypes.c_int32) for name in ("product", "row_begin", "row_count", "reserved2")] + [
        ("d_out", ctypes.c_void_p)]


class MwrtObsApply(ctypes.Structure):
    """include/mwrt.h mwrt_obs_apply: the record of one application of an instrument operator (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("d_tb_in", ctypes.c_void_p), ("d_tb_out", ctypes.c_void_p), ("d_k_in", ctypes.c_void_p * 4),
                ("d_k_out", ctypes.c_void_p * 4)]


class MwrtBasisApply(ctypes.Structure):
    """include/mwrt.h mwrt_basis_apply: the record of one projection onto, or expansion from, a reduced basis (device
    pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_int32), ("d_k_in", ctypes.c_void_p * 4),
                ("d_k_out", ctypes.c_void_p), ("d_c", ctypes.c_void_p), ("d_x_ref", ctypes.c_void_p),
                ("d_x", ctypes.c_void_p), ("x_ref_per_profile", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


class MwrtObsWhiten(ctypes.Structure):
    """include/mwrt.h mwrt_obs_whiten: the record of one pre-whitening with a per-profile observation-error covariance, or
    of one application of its stored factor (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nblk", ctypes.c_int32), ("se_full", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("reserved", ctypes.c_int64), ("d_se", ctypes.c_void_p), ("d_y", ctypes.c_void_p),
                ("d_fx", ctypes.c_void_p), ("d_k_in", ctypes.c_void_p * 4), ("d_l", ctypes.c_void_p),
                ("d_keep", ctypes.c_void_p), ("d_status", ctypes.c_void_p), ("d_y_out", ctypes.c_void_p),
                ("d_fx_out", ctypes.c_void_p), ("d_k_out", ctypes.c_void_p * 4)]


#: include/mwrt.h mwrt_obs_whiten.mode: L^-1 (whitening) and L^-T (the gain back to d x^ / d y)
WHITEN_FORWARD, WHITEN_TRANSPOSED = 0, 1

#: include/mwrt.h MWRT_OE_PRODUCT_*: what mwrt_oe_product_device forms
OE_PRODUCT_AVK, OE_PRODUCT_POST_COV = 0, 1

class MwrtParam(ctypes.Structure):
    """include/mwrt.h mwrt_param: one spectroscopic parameter, a (field, line) pair."""
    _fields_ = [("field", ctypes.c_int32), ("line", ctypes.c_int32)]


#: include/mwrt.h MWRT_MAX_PARAMS, MWRT_PAR_ALL_LINES and the MWRT_PAR_* field ids, by the ModelTables name of the entry
MAX_PARAMS = 256
PAR_ALL_LINES = -1
PARAM_FIELDS = {name: i for i, name in enumerate((
    "h2o_cf", "h2o_cs", "h2o_xcf", "h2o_xcs", "o2_x", "o2_wb300", "n2_l",
    "h2o_s1", "h2o_b2", "h2o_w0", "h2o_x", "h2o_w0s", "h2o_xs", "h2o_sh", "h2o_shs",
    "o2_s300", "o2_be", "o2_w300", "o2_y0", "o2_y1", "o2_g0", "o2_g1", "o2_dnu0", "o2_dnu1"))}
PAR_FIRST_H2O_LINE_FIELD = PARAM_FIELDS["h2o_s1"]      # below it: scalar fields (line must be 0)
PAR_FIRST_O2_LINE_FIELD = PARAM_FIELDS["o2_s300"]


def _params(params):
    """A sequence of ``MwrtParam`` / (field, line) pairs -> a ctypes array the native call reads."""
    arr = (MwrtParam * len(params))()
    for i, q in enumerate(params):
        arr[i].field, arr[i].line = (q.field, q.line) if isinstance(q, MwrtParam) else (int(q[0]), int(q[1]))
    return arr


#: include/mwrt.h MWRT_OE_MAX_M: observations per profile of one optimal-estimation step
OE_MAX_M = 140

#: include/mwrt.h MWRT_OE_NFORM_MAX_N: state elements per profile of one n-form step (its m is not bounded)
OE_NFORM_MAX_N = 128

#: include/mwrt.h MWRT_MAX_ANGLES: elevations of one forward-operator call
MAX_ANGLES = 64

MWRT_VERSION = 301
#: MWRT_HELPER_* of include/mwrt.h (mwrt_selftest_helpers), in the header's order
HELPERS = {name: k for k, name in enumerate((
    "fexp_small", "fexp_tiny", "ftanh_half_small", "ftanh_half_tiny", "two_atanh_tail", "fsqrt", "crecip", "cmul_cdiv",
    "csqrt_principal", "dcerror_upper", "hui_w_dw", "planck_b", "layer_value_zf1", "layer_value_zf0", "layer_value4",
    "layer_value_tl_zf1", "layer_value_tl_zf0", "div_small", "block_sum", "block_scan", "block_suffix_excl", "row16_max",
    "wave_votes"))}


#: every symbol include/mwrt.h declares: (name, restype, argtypes)
_i32, _i64, _vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
SIGNATURES = {
    "mwrt_version": (ctypes.c_int, []),
    "mwrt_model_desc_size": (ctypes.c_size_t, []),
    "mwrt_device_count": (ctypes.c_int, []),
    "mwrt_last_error": (ctypes.c_char_p, []),
    "mwrt_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "mwrt_destroy": (ctypes.c_int, [_vp]),
    "mwrt_model_create": (ctypes.c_int, [_vp, ctypes.POINTER(MwrtModelDesc), ctypes.POINTER(_vp)]),
    "mwrt_model_destroy": (ctypes.c_int, [_vp, _vp]),
    "mwrt_tb_batch": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                     _vp, _vp, ctypes.POINTER(MwrtTbExtras)]),
    "mwrt_tb_batch_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                            _vp, _vp, ctypes.POINTER(MwrtTbExtras), _vp]),
    "mwrt_tb_batch_opt": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                         _vp, _vp, ctypes.POINTER(MwrtTbExtras), ctypes.POINTER(MwrtTbOptions)]),
    "mwrt_tb_batch_opt_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                _vp, _vp, ctypes.POINTER(MwrtTbExtras), ctypes.POINTER(MwrtTbOptions),
                                                _vp]),
    "mwrt_tb_from_absorption_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp,
                                                      _vp, _vp, _vp]),
    "mwrt_tb_batch_multi": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(_vp), _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                           _i32, _vp, _vp, _vp]),
    "mwrt_tb_batch_multi_device": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(_vp), _i64, _i32, _vp, _vp, _vp, _vp, _i32,
                                                  _vp, _i32, _vp, _vp, _vp, _vp]),
    "mwrt_absorption_batch": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mwrt_absorption_batch_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mwrt_layer_tau_pitch": (ctypes.c_int, [_i32]),
    "mwrt_layer_tau_batch_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mwrt_tb_from_layer_tau_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp,
                                                     _vp]),
    "mwrt_tb_jacobian_batch": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp,
                                              _vp, _vp]),
    "mwrt_absorption_tl_batch_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                                       _vp, _vp, _vp]),
    "mwrt_tb_jacobian_batch_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp,
                                                     _vp, _vp, _vp, _vp, _vp]),
    "mwrt_tb_jacobian_batch_opt_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(MwrtTbOptions),
                                                         _vp]),
    "mwrt_tb_jacobian_batch_vars_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(MwrtTbOptions),
                                                          ctypes.POINTER(JacVariables), _vp]),
    "mwrt_tb_jacobian_batch_vars": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(MwrtTbOptions),
                                                   ctypes.POINTER(JacVariables)]),
    "mwrt_tb_jacobian_batch_ray_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(MwrtTbOptions),
                                                         ctypes.POINTER(JacVariables), _vp]),
    "mwrt_tb_jacobian_batch_ray": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(MwrtTbOptions),
                                                  ctypes.POINTER(JacVariables)]),
    "mwrt_tb_param_jacobian_batch_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                           _i32, ctypes.POINTER(MwrtParam), _vp, _vp, _vp, _vp]),
    "mwrt_tb_param_jacobian_batch": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                                    _i32, ctypes.POINTER(MwrtParam), _vp, _vp, _vp]),
    "mwrt_oe_step_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeStep), _vp]),
    "mwrt_oe_step_size": (ctypes.c_size_t, []),
    "mwrt_oe_lm_prepare_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeLm), _vp]),
    "mwrt_oe_lm_solve_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeLm), _vp]),
    "mwrt_oe_cost_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeLm), _vp]),
    "mwrt_oe_lm_size": (ctypes.c_size_t, []),
    "mwrt_oe_nform_prepare_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeNform), _vp]),
    "mwrt_oe_nform_solve_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeNform), _vp]),
    "mwrt_oe_nform_cost_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeNform), _vp]),
    "mwrt_oe_nform_size": (ctypes.c_size_t, []),
    "mwrt_oe_nform_char_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeNformChar), _vp]),
    "mwrt_oe_nform_gain_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeNformChar), _vp]),
    "mwrt_oe_nform_char_size": (ctypes.c_size_t, []),
    "mwrt_oe_select_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeSelect), _vp]),
    "mwrt_oe_select_size": (ctypes.c_size_t, []),
    "mwrt_oe_gain_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeChar), _vp]),
    "mwrt_oe_product_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtOeChar), _vp]),
    "mwrt_oe_char_size": (ctypes.c_size_t, []),
    "mwrt_obs_create": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, ctypes.POINTER(_vp)]),
    "mwrt_obs_destroy": (ctypes.c_int, [_vp]),
    "mwrt_obs_apply_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, ctypes.POINTER(MwrtObsApply), _vp]),
    "mwrt_obs_apply_size": (ctypes.c_uint32, []),
    "mwrt_basis_create": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, ctypes.POINTER(_vp)]),
    "mwrt_basis_destroy": (ctypes.c_int, [_vp]),
    "mwrt_basis_project_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, ctypes.POINTER(MwrtBasisApply), _vp]),
    "mwrt_basis_expand_device": (ctypes.c_int, [_vp, _vp, _i64, ctypes.POINTER(MwrtBasisApply), _vp]),
    "mwrt_basis_apply_size": (ctypes.c_uint32, []),
    "mwrt_obs_whiten_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtObsWhiten), _vp]),
    "mwrt_obs_whiten_apply_device": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(MwrtObsWhiten), _vp]),
    "mwrt_obs_whiten_size": (ctypes.c_uint32, []),
    "mwrt_set_absorption_mode": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mwrt_set_chunk_width": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mwrt_selftest_math": (ctypes.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mwrt_selftest_helpers": (ctypes.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 9),
    "mwrt_synchronize": (ctypes.c_int, [_vp, _vp]),
    "mwrt_set_timing": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mwrt_timing_collect": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]),
    "mwrt_last_kernel_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double)]),
}

#: (record of include/mwrt.h, its ctypes structure, the file that declares it): ``<record>_size()`` must agree with each
_RECORD_SIZES = (
    ("mwrt_model_desc", MwrtModelDesc, "spectroscopy.py"), ("mwrt_oe_step", MwrtOeStep, "_native.py"),
    ("mwrt_oe_lm", MwrtOeLm, "_native.py"), ("mwrt_oe_nform", MwrtOeNform, "_native.py"),
    ("mwrt_oe_nform_char", MwrtOeNformChar, "_native.py"), ("mwrt_oe_select", MwrtOeSelect, "_native.py"),
    ("mwrt_oe_char", MwrtOeChar, "_native.py"),
    ("mwrt_obs_apply", MwrtObsApply, "_native.py"), ("mwrt_basis_apply", MwrtBasisApply, "_native.py"),
    ("mwrt_obs_whiten", MwrtObsWhiten, "_native.py"))

_lib = None
_lib_lock = threading.Lock()
_hip_runtime_path = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7) and asks for it by the bare file name, so if libmwrt.so pulled in the
    system copy first, a later ``import torch`` would load a second runtime and find no GPU.
    Pre-loading torch's copy (when torch is installed) makes libmwrt.so's DT_NEEDED
    ``libamdhip64.so.7`` resolve to the same object whatever the import order."""
    global _hip_runtime_path
    if _hip_runtime_path is not None:
        return
    _hip_runtime_path = ""
    if os.environ.get("MWRT_SYSTEM_HIP", "0") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        _hip_runtime_path = cand


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen libmwrt.so and type every entry point.  Raises NativeLibraryMissing if absent."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or os.environ.get("MWRT_LIB") or LIB_PATH      # MWRT_LIB: diagnostic builds only
        if not os.path.exists(p):
            raise NativeLibraryMissing(
                f"{p} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _share_hip_runtime_with_torch()
        lib = ctypes.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        for name, struct, where in _RECORD_SIZES:
            if getattr(lib, name + "_size")() != ctypes.sizeof(struct):
                raise NativeLibraryMissing(f"{name} layout mismatch between libmwrt.so and {where}")
        if lib.mwrt_version() != MWRT_VERSION:
            raise NativeLibraryMissing(f"libmwrt.so is version {lib.mwrt_version()}, this binding needs {MWRT_VERSION}: "
                                       "rebuild (python -c 'import __graft_entry__ as g; g.build()')")
        if path is None:
            _lib = lib
        return lib


def device_count() -> int:
    return int(load_library().mwrt_device_count())


def _f64(a, shape=None, name="array"):
    """Contiguous float64 copy/view; resolves the negative-stride views the wrapper passes
    (z_in[::-1], PyRTlib_processing.py:123)."""
    x = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and x.shape != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {x.shape}")
    return x


def _ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p) if isinstance(x, np.ndarray) else ctypes.c_void_p(int(x))


def _profile_args(z, p, t, rh, frq, elev):
    """What the host-buffer entries share: contiguous [nprof][nlev] profiles and flat frequency / elevation lists."""
    z = _f64(z)
    if z.ndim != 2:
        raise ValueError("profiles must be [nprof][nlev]")
    return z, _f64(p, z.shape, "p"), _f64(t, z.shape, "t"), _f64(rh, z.shape, "rh"), _f64(frq).ravel(), _f64(elev).ravel()


def _options(denliq=None, denice=None, ray_tracing=False, o3n=None):
    """The ``MwrtTbOptions`` of the opt-in physics (NumPy arrays, which the caller keeps alive, or device addresses), or
    None when nothing is opted into."""
    if denliq is None and denice is None and not ray_tracing and o3n is None:
        return None
    addr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else int(x)   # noqa: E731
    return MwrtTbOptions(addr(denliq), addr(denice), int(bool(ray_tracing)), 0, addr(o3n))


#: include/mwrt.h MWRT_STREAM_LEGACY: the caller's legacy default stream (hipStream_t 0)
STREAM_LEGACY = ctypes.c_void_p(-1).value


def _stream(stream):
    """`stream` argument of the *_device entry points -> the ABI's void*.

    None = the context's own non-blocking stream (ABI NULL); 0 = the legacy default stream --
    what ``torch.cuda.current_stream().cuda_stream`` returns for torch's default stream -- passed
    as MWRT_STREAM_LEGACY so the launch is ordered with the caller's other default-stream work;
    any other integer is a hipStream_t handle."""
    if stream is None:
        return None
    stream = int(stream)
    return ctypes.c_void_p(STREAM_LEGACY if stream == 0 else stream)


def _record(cls, struct_size, ints, ptrs, **blocks):
    """A record of the structure ``cls`` as every record entry is handed one: ``struct_size`` (None: the whole record), the
    integer fields ``ints``, the device pointers ``ptrs`` (None: NULL) and, for each pointer array ``blocks`` names, its
    first four entries.  Whatever is not named stays 0 / NULL."""
    rec = cls()
    rec.struct_size = ctypes.sizeof(cls) if struct_size is None else int(struct_size)
    for name, v in ints.items():
        setattr(rec, name, int(v or 0))
    for name, v in ptrs.items():
        setattr(rec, name, None if v is None else int(v))
    for name, seq in blocks.items():
        for b, k in enumerate(list(seq)[:4]):
            getattr(rec, name)[b] = None if k is None else int(k)
    return rec


def _serialised(method):
    """A native context owns one workspace and one stream: calls from several Python threads are
    serialised per context (ctypes drops the GIL during the call)."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return method(self, *args, **kwargs)
    return wrapper


class Context:
    """One (host thread, GPU) pair: HIP stream + workspace + cached model tables."""

    def __init__(self, device_id: int = 0):
        self._lock = threading.RLock()
        self._lib = load_library()
        h = ctypes.c_void_p()
        self._handle = None
        self._check(self._lib.mwrt_create(int(device_id), ctypes.byref(h)), "mwrt_create")
        self._handle = h
        self.device_id = int(device_id)
        # device tables per ModelTables OBJECT (keyed by identity, the record kept alive beside its
        # handle): two different records may share a name, and a handle is never destroyed while
        # the context lives -- a queued launch or another caller may still hold it
        self._models: Dict[int, tuple] = {}

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc: int, where: str):
        if rc != 0:
            raise MwrtError(rc, where, self._lib.mwrt_last_error().decode("utf-8", "replace"))

    @_serialised
    def close(self):
        if getattr(self, "_handle", None):
            for m, _tables in self._models.values():
                self._lib.mwrt_model_destroy(self._handle, m)
            self._models.clear()
            self._lib.mwrt_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @_serialised
    def model(self, model) -> ctypes.c_void_p:
        """Device-resident tables for a model name or a ModelTables record (cached per context)."""
        tables = get_model(model) if isinstance(model, str) else model
        hit = self._models.get(id(tables))
        if hit is not None:
            return hit[0]
        desc = tables.to_c()
        h = ctypes.c_void_p()
        self._check(self._lib.mwrt_model_create(self._handle, ctypes.byref(desc), ctypes.byref(h)), "mwrt_model_create")
        self._models[id(tables)] = (h, tables)
        return h

    # -- host-buffer entry points ------------------------------------------------------------
    @_serialised
    def tb_batch(self, model, z, p, t, rh, frq, elev, extras=False, denliq=None, denice=None, ray_tracing=False, o3n=None):
        """[nprof][nlev] profiles (ground->top) -> tb [nprof][nang][nf], valid [nprof] (+ extras dict).

        ``denliq`` / ``denice`` ([nprof][nlev], g m-3), ``ray_tracing`` and ``o3n`` ([nprof][nlev], molecules m-3; the
        model must carry an extra-species line table) are the opt-in physics of ``mwrt_tb_options``; left at their
        defaults the call is the reference's clear-sky plane-parallel path."""
        z, p, t, rh, frq, elev = _profile_args(z, p, t, rh, frq, elev)
        nprof, nlev = z.shape
        nf, nang = frq.size, elev.size
        tb = np.empty((nprof, nang, nf))
        valid = np.empty(nprof, dtype=np.uint8)
        ex, exs = None, None
        if extras:
            ex = {k: np.empty((nprof, nang, nf)) for k in ("tbatm", "tmr", "tauwet", "taudry", "tauliq", "tauice")}
            ex["taulay"] = np.empty((nprof, nf, nlev))
            exs = MwrtTbExtras(*[ex[k].ctypes.data for k in ("tbatm", "tmr", "tauwet", "taudry", "taulay", "tauliq",
                                                              "tauice")])
        dl = None if denliq is None else _f64(denliq, z.shape, "denliq")
        di = None if denice is None else _f64(denice, z.shape, "denice")
        do3 = None if o3n is None else _f64(o3n, z.shape, "o3n")
        opts = _options(dl, di, ray_tracing, do3)
        self._check(self._lib.mwrt_tb_batch_opt(
            self._handle, self.model(model), nprof, nlev, _ptr(z), _ptr(p), _ptr(t), _ptr(rh),
            nf, _ptr(frq), nang, _ptr(elev), _ptr(tb), _ptr(valid),
            ctypes.byref(exs) if exs is not None else None,
            ctypes.byref(opts) if opts is not None else None), "mwrt_tb_batch_opt")
        return (tb, valid, ex) if extras else (tb, valid)

    @_serialised
    def tb_batch_multi(self, models, z, p, t, rh, frq, elev):
        """Several models over the same profiles in ONE launch: tb [nmodels][nprof][nang][nf], valid [nmodels][nprof]."""
        z, p, t, rh, frq, elev = _profile_args(z, p, t, rh, frq, elev)
        nprof, nlev = z.shape
        handles = (ctypes.c_void_p * len(models))(*[self.model(m) for m in models])
        tb = np.empty((len(models), nprof, elev.size, frq.size))
        valid = np.empty((len(models), nprof), dtype=np.uint8)
        self._check(self._lib.mwrt_tb_batch_multi(
            self._handle, len(models), handles, nprof, nlev, _ptr(z), _ptr(p), _ptr(t), _ptr(rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(tb), _ptr(valid)), "mwrt_tb_batch_multi")
        return tb, valid

    @_serialised
    def tb_batch_multi_device(self, models, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_valid, stream=None):
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        handles = (ctypes.c_void_p * len(models))(*[self.model(m) for m in models])
        self._check(self._lib.mwrt_tb_batch_multi_device(
            self._handle, len(models), handles, int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(d_tb), _ptr(d_valid),
            _stream(stream)), "mwrt_tb_batch_multi_device")

    @_serialised
    def absorption_batch(self, model, p, t, rh, frq):
        """-> awet, adry [nprof][nf][nlev] in Np/km."""
        p = _f64(p)
        nprof, nlev = p.shape
        t, rh = _f64(t, p.shape, "t"), _f64(rh, p.shape, "rh")
        frq = _f64(frq).ravel()
        awet = np.empty((nprof, frq.size, nlev))
        adry = np.empty_like(awet)
        self._check(self._lib.mwrt_absorption_batch(
            self._handle, self.model(model), nprof, nlev, _ptr(p), _ptr(t), _ptr(rh),
            frq.size, _ptr(frq), _ptr(awet), _ptr(adry)), "mwrt_absorption_batch")
        return awet, adry

    @_serialised
    def tb_jacobian_batch(self, model, z, p, t, rh, frq, elev):
        """K-matrix in one call, what include/mwrt.h's mwrt_tb_jacobian_batch computes: ``tb_jacobian_batch_vars`` in the
        operator's own variables.  Returns ``tb [nprof][nang][nf]``, ``valid`` and a dict of ``dtb_dt`` [K/K at fixed e],
        ``dtb_de`` [K/hPa], ``dtb_ddz`` [K/km of layer thickness], each ``[nprof][nang][nf][nlev]`` (levels ground -> top)."""
        tb, valid, jac = self.tb_jacobian_batch_vars(model, z, p, t, rh, frq, elev)
        jac["dtb_de"] = jac.pop("dtb_dh")
        return tb, valid, jac

    # -- device-buffer entry points (raw device addresses, e.g. torch.Tensor.data_ptr()) -------
    @_serialised
    def tb_batch_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_valid,
                        extras: Optional[MwrtTbExtras] = None, stream=None, d_denliq=None, d_denice=None,
                        ray_tracing=False, d_o3n=None):
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        opts = _options(d_denliq, d_denice, ray_tracing, d_o3n)
        if opts is None:
            self._check(self._lib.mwrt_tb_batch_device(
                self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
                frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(d_tb), _ptr(d_valid),
                ctypes.byref(extras) if extras is not None else None,
                _stream(stream)), "mwrt_tb_batch_device")
            return
        self._check(self._lib.mwrt_tb_batch_opt_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(d_tb), _ptr(d_valid),
            ctypes.byref(extras) if extras is not None else None, ctypes.byref(opts),
            _stream(stream)), "mwrt_tb_batch_opt_device")

    @_serialised
    def tb_from_absorption_device(self, model, nprof, nlev, d_z, d_t, frq, elev, d_awet, d_adry, d_tb, d_valid, stream=None):
        """Layer integration + RTE from absorption coefficients already in HBM ([nprof][nf][nlev], as
        absorption_batch_device writes them): the K2 half of the K1 -> alpha -> K2 two-kernel form."""
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        self._check(self._lib.mwrt_tb_from_absorption_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_t), frq.size, _ptr(frq),
            elev.size, _ptr(elev), _ptr(d_awet), _ptr(d_adry), _ptr(d_tb), _ptr(d_valid), _stream(stream)),
            "mwrt_tb_from_absorption_device")

    @_serialised
    def absorption_batch_device(self, model, nprof, nlev, d_p, d_t, d_rh, frq, d_awet, d_adry, stream=None):
        frq = _f64(frq).ravel()
        self._check(self._lib.mwrt_absorption_batch_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), _ptr(d_awet), _ptr(d_adry),
            _stream(stream)), "mwrt_absorption_batch_device")

    @_serialised
    def absorption_tl_batch_device(self, model, nprof, nlev, d_p, d_t, d_rh, frq, d_awet, d_adry, d_dawet_dt, d_dawet_de,
                                   d_dadry_dt, d_dadry_de, stream=None):
        """Tangent-linear absorption (include/mwrt.h mwrt_absorption_tl_batch_device): awet, adry [Np/km] and their partial
        derivatives with respect to T at fixed e [Np/km/K] and e at fixed T [Np/km/hPa], each [nprof][nf][nlev]."""
        frq = _f64(frq).ravel()
        self._check(self._lib.mwrt_absorption_tl_batch_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_p), _ptr(d_t), _ptr(d_rh), frq.size, _ptr(frq),
            _ptr(d_awet), _ptr(d_adry), _ptr(d_dawet_dt), _ptr(d_dawet_de), _ptr(d_dadry_dt), _ptr(d_dadry_de),
            _stream(stream)), "mwrt_absorption_tl_batch_device")

    @_serialised
    def tb_jacobian_batch_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_dtb_dt, d_dtb_de,
                                 d_dtb_ddz, d_valid, stream=None):
        """The K-matrix on device buffers (include/mwrt.h mwrt_tb_jacobian_batch_device): tb [nprof][nang][nf], dtb_dt,
        dtb_de, dtb_ddz [nprof][nang][nf][nlev] and valid [nprof], as ``tb_jacobian_batch`` returns them."""
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        self._check(self._lib.mwrt_tb_jacobian_batch_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(d_tb), _ptr(d_dtb_dt), _ptr(d_dtb_de), _ptr(d_dtb_ddz),
            _ptr(d_valid), _stream(stream)), "mwrt_tb_jacobian_batch_device")

    @_serialised
    def tb_jacobian_batch_opt_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_dtb_dt, d_dtb_de,
                                     d_dtb_ddz, d_valid, d_denliq=None, d_denice=None, d_dtb_dliq=None, d_dtb_dice=None,
                                     stream=None, ray_tracing=False, d_o3n=None):
        """The K-matrix under cloud liquid / ice (include/mwrt.h mwrt_tb_jacobian_batch_opt_device): as
        ``tb_jacobian_batch_device`` with ``d_denliq`` / ``d_denice`` [nprof][nlev] (g m-3) as inputs and ``d_dtb_dliq`` /
        ``d_dtb_dice`` [nprof][nang][nf][nlev] (K per g m-3) as further outputs; each may be None.  ``ray_tracing`` and
        ``d_o3n`` exist to be refused (MWRT_ERR_UNSUPPORTED)."""
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        opts = _options(d_denliq, d_denice, ray_tracing, d_o3n)
        self._check(self._lib.mwrt_tb_jacobian_batch_opt_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(d_tb), _ptr(d_dtb_dt), _ptr(d_dtb_de), _ptr(d_dtb_ddz),
            _ptr(d_dtb_dliq) if d_dtb_dliq is not None else None, _ptr(d_dtb_dice) if d_dtb_dice is not None else None,
            _ptr(d_valid), ctypes.byref(opts) if opts is not None else None, _stream(stream)),
            "mwrt_tb_jacobian_batch_opt_device")

    @_serialised
    def tb_jacobian_batch_vars_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_dtb_dt, d_dtb_dh,
                                      d_valid, d_dtb_ddz=None, d_denliq=None, d_denice=None, d_dtb_dliq=None,
                                      d_dtb_dice=None, variables=None, stream=None, ray_tracing=False, d_o3n=None):
        """The device K-matrix in retrieval variables (include/mwrt.h mwrt_tb_jacobian_batch_vars_device): as
        ``tb_jacobian_batch_opt_device`` with ``variables`` a ``JacVariables`` (None: the raw rows) and ``d_dtb_ddz``
        optional in every mode.  ``d_dtb_dh`` receives the humidity row in the variable asked for."""
        self._jacobian_vars_device("mwrt_tb_jacobian_batch_vars_device", model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev,
                                   d_tb, d_dtb_dt, d_dtb_dh, d_valid, d_dtb_ddz, _options(d_denliq, d_denice, ray_tracing, d_o3n),
                                   d_dtb_dliq, d_dtb_dice, variables, stream)

    def _jacobian_vars_device(self, symbol, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_dtb_dt, d_dtb_dh,
                              d_valid, d_dtb_ddz, opts, d_dtb_dliq, d_dtb_dice, variables, stream):
        """The one parameter list mwrt_tb_jacobian_batch_vars_device and mwrt_tb_jacobian_batch_ray_device share."""
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        opt_ptr = lambda x: _ptr(x) if x is not None else None   # noqa: E731
        self._check(getattr(self._lib, symbol)(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), _ptr(d_tb), _ptr(d_dtb_dt), _ptr(d_dtb_dh), opt_ptr(d_dtb_ddz),
            opt_ptr(d_dtb_dliq), opt_ptr(d_dtb_dice), _ptr(d_valid), ctypes.byref(opts) if opts is not None else None,
            ctypes.byref(variables) if variables is not None else None, _stream(stream)), symbol)

    @_serialised
    def tb_jacobian_batch_ray_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, d_tb, d_dtb_dt, d_dtb_dh,
                                     d_valid, d_dtb_ddz=None, d_denliq=None, d_denice=None, d_dtb_dliq=None,
                                     d_dtb_dice=None, variables=None, stream=None):
        """The device K-matrix along refracted spherical ray paths (include/mwrt.h mwrt_tb_jacobian_batch_ray_device): the
        K-matrix of ``tb_batch_device(ray_tracing=True)``, rows exact (the path's response to the state included), in the
        layout and with the keywords of ``tb_jacobian_batch_vars_device``.  ``valid`` is 3 where a ray was trapped."""
        self._jacobian_vars_device("mwrt_tb_jacobian_batch_ray_device", model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev,
                                   d_tb, d_dtb_dt, d_dtb_dh, d_valid, d_dtb_ddz, _options(d_denliq, d_denice), d_dtb_dliq,
                                   d_dtb_dice, variables, stream)

    @_serialised
    def tb_jacobian_batch_ray(self, model, z, p, t, rh, frq, elev, denliq=None, denice=None, variables=None,
                              thickness=True):
        """The same on NumPy arrays, synchronous (include/mwrt.h mwrt_tb_jacobian_batch_ray): what
        ``tb_jacobian_batch_vars`` returns, along ray-traced paths."""
        return self._jacobian_vars_host("mwrt_tb_jacobian_batch_ray", model, z, p, t, rh, frq, elev, denliq, denice,
                                        variables, thickness)

    @_serialised
    def tb_jacobian_batch_vars(self, model, z, p, t, rh, frq, elev, denliq=None, denice=None, variables=None,
                               thickness=True):
        """The same on NumPy arrays, synchronous (include/mwrt.h mwrt_tb_jacobian_batch_vars): returns ``tb
        [nprof][nang][nf]``, ``valid [nprof]`` and a dict of ``dtb_dt``, ``dtb_dh`` (the humidity row in the variable
        asked for), ``dtb_ddz`` (the raw thickness row; absent with ``thickness=False``) and, for each cloud array given,
        ``dtb_dliq`` / ``dtb_dice``, each ``[nprof][nang][nf][nlev]`` (levels ground -> top)."""
        return self._jacobian_vars_host("mwrt_tb_jacobian_batch_vars", model, z, p, t, rh, frq, elev, denliq, denice,
                                        variables, thickness)

    def _jacobian_vars_host(self, symbol, model, z, p, t, rh, frq, elev, denliq, denice, variables, thickness):
        """The one parameter list mwrt_tb_jacobian_batch_vars and mwrt_tb_jacobian_batch_ray share."""
        z, p, t, rh, frq, elev = _profile_args(z, p, t, rh, frq, elev)
        nprof, nlev = z.shape
        nf, nang = frq.size, elev.size
        dl = None if denliq is None else _f64(denliq, z.shape, "denliq")
        di = None if denice is None else _f64(denice, z.shape, "denice")
        opts = _options(dl, di)
        keys = ["dtb_dt", "dtb_dh"] + (["dtb_ddz"] if thickness else []) + (["dtb_dliq"] if dl is not None else []) + \
               (["dtb_dice"] if di is not None else [])
        tb = np.empty((nprof, nang, nf))
        jac = {k: np.empty((nprof, nang, nf, nlev)) for k in keys}
        valid = np.empty(nprof, dtype=np.uint8)
        out = [_ptr(jac[k]) if k in jac else None for k in ("dtb_dt", "dtb_dh", "dtb_ddz", "dtb_dliq", "dtb_dice")]
        self._check(getattr(self._lib, symbol)(
            self._handle, self.model(model), nprof, nlev, _ptr(z), _ptr(p), _ptr(t), _ptr(rh), nf, _ptr(frq), nang, _ptr(elev),
            _ptr(tb), *out, _ptr(valid), ctypes.byref(opts) if opts is not None else None,
            ctypes.byref(variables) if variables is not None else None), symbol)
        return tb, valid, jac

    @_serialised
    def tb_param_jacobian_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, elev, params, d_dtb_db, d_valid,
                                 d_tb=None, stream=None):
        """The spectroscopic-parameter Jacobian on device buffers (include/mwrt.h mwrt_tb_param_jacobian_batch_device):
        ``params`` is a sequence of ``MwrtParam`` or (field, line) pairs, ``d_dtb_db`` [nprof][nang][nf][npar] (parameter
        fastest, K per unit of the table entry), ``d_valid`` [nprof] and the optional ``d_tb`` [nprof][nang][nf]."""
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        arr = _params(params)
        self._check(self._lib.mwrt_tb_param_jacobian_batch_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), elev.size, _ptr(elev), len(arr), arr, _ptr(d_tb) if d_tb is not None else None,
            _ptr(d_dtb_db), _ptr(d_valid), _stream(stream)), "mwrt_tb_param_jacobian_batch_device")

    @_serialised
    def tb_param_jacobian(self, model, z, p, t, rh, frq, elev, params):
        """The same on NumPy arrays, synchronous (include/mwrt.h mwrt_tb_param_jacobian_batch): returns ``tb
        [nprof][nang][nf]``, ``dtb_db [nprof][nang][nf][npar]`` and ``valid [nprof]``."""
        z, p, t, rh, frq, elev = _profile_args(z, p, t, rh, frq, elev)
        nprof, nlev = z.shape
        arr = _params(params)
        tb = np.empty((nprof, elev.size, frq.size))
        kb = np.empty((nprof, elev.size, frq.size, len(arr)))
        valid = np.empty(nprof, dtype=np.uint8)
        self._check(self._lib.mwrt_tb_param_jacobian_batch(
            self._handle, self.model(model), nprof, nlev, _ptr(z), _ptr(p), _ptr(t), _ptr(rh), frq.size, _ptr(frq),
            elev.size, _ptr(elev), len(arr), arr, _ptr(tb), _ptr(kb), _ptr(valid)), "mwrt_tb_param_jacobian_batch")
        return tb, kb, valid

    @_serialised
    def oe_step_device(self, nprof, nlev, m, d_k, d_x, d_xa, d_sa, d_se, d_y, d_fx, d_x_new, d_status, d_chi2=None,
                       d_dfs=None, d_post_var=None, d_nobs=None, xa_per_profile=False, se_full=False, stream=None,
                       reserved=0, struct_size=None):
        """One optimal-estimation step per profile (include/mwrt.h mwrt_oe_step_device): ``d_k`` is the sequence of the
        1 .. 4 K-matrix blocks ``[nprof][m][nlev]`` (Jacobian outputs as they were written), the state, prior and
        covariances as the header lays them out; ``d_x_new [nprof][nblk][nlev]`` and ``d_status [nprof]`` (uint8) are
        required, the diagnostics optional.  ``struct_size`` (default: the whole record) is what the record claims."""
        self._oe(MwrtOeStep, "mwrt_oe_step_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_full=bool(se_full), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_sa=d_sa, d_se=d_se, d_y=d_y, d_fx=d_fx, d_x_new=d_x_new, d_status=d_status,
                      d_chi2=d_chi2, d_dfs=d_dfs, d_post_var=d_post_var, d_nobs=d_nobs))

    def _oe(self, cls, entry, nprof, nlev, m, d_k, stream, struct_size, ints, ptrs):
        """The one call of the optimal-estimation entries: a record of ``cls`` (``_record``) with ``nblk = len(d_k)``, the
        integer fields ``ints`` and the pointers ``ptrs``, handed to ``entry(ctx, nprof, nlev, m, record, stream)``."""
        d_k = list(d_k)
        rec = _record(cls, struct_size, dict(ints, nblk=len(d_k)), ptrs, d_k=d_k)
        self._check(getattr(self._lib, entry)(self._handle, int(nprof), int(nlev), int(m), ctypes.byref(rec), _stream(stream)),
                    entry)

    @_serialised
    def oe_lm_prepare_device(self, nprof, nlev, m, d_k, d_x, d_xa, d_sa, d_se, d_y, d_fx, d_g0, d_r, d_kdx, d_keep,
                             d_lin_status, d_active=None, xa_per_profile=False, se_full=False, stream=None, reserved=0,
                             struct_size=None):
        """The linearisation at x (include/mwrt.h mwrt_oe_lm_prepare_device): the inputs of ``oe_step_device``; writes
        ``d_g0 [nprof][m (m + 1) / 2]``, ``d_r`` and ``d_kdx [nprof][m]``, ``d_keep [nprof][m]`` and ``d_lin_status [nprof]``
        (uint8).  A profile whose ``d_active`` flag (uint8, optional) is 0 is skipped."""
        self._oe(MwrtOeLm, "mwrt_oe_lm_prepare_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_full=bool(se_full), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_sa=d_sa, d_se=d_se, d_y=d_y, d_fx=d_fx, d_g0=d_g0, d_r=d_r, d_kdx=d_kdx,
                      d_keep=d_keep, d_lin_status=d_lin_status, d_active=d_active))

    @_serialised
    def oe_lm_solve_device(self, nprof, nlev, m, d_k, d_x, d_xa, d_sa, d_se, d_gamma, d_g0, d_r, d_kdx, d_keep,
                           d_lin_status, d_x_new, d_status, d_chi2=None, d_nobs=None, d_active=None, xa_per_profile=False,
                           se_full=False, stream=None, reserved=0, struct_size=None):
        """One damped trial on a linearisation (include/mwrt.h mwrt_oe_lm_solve_device) with ``d_gamma [nprof]``:
        ``d_x_new [nprof][nblk][nlev]`` and ``d_status [nprof]`` (uint8) required, ``d_chi2`` and ``d_nobs`` optional."""
        self._oe(MwrtOeLm, "mwrt_oe_lm_solve_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_full=bool(se_full), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_sa=d_sa, d_se=d_se, d_gamma=d_gamma, d_g0=d_g0, d_r=d_r, d_kdx=d_kdx,
                      d_keep=d_keep, d_lin_status=d_lin_status, d_x_new=d_x_new, d_status=d_status, d_chi2=d_chi2,
                      d_nobs=d_nobs, d_active=d_active))

    @_serialised
    def oe_cost_device(self, nprof, nlev, m, nblk, d_x, d_xa, d_se, d_y, d_fx, d_keep, d_sa_inv, d_cost, d_cost_obs=None,
                       d_cost_prior=None, d_status=None, d_active=None, xa_per_profile=False, se_full=False, stream=None,
                       reserved=0, struct_size=None):
        """J = r^T Se^-1 r over the rows ``d_keep`` names + (x - xa)^T Sa^-1 (x - xa) (include/mwrt.h mwrt_oe_cost_device);
        ``nblk`` is the number of state blocks (the call reads no K)."""
        self._oe(MwrtOeLm, "mwrt_oe_cost_device", nprof, nlev, m, [None] * int(nblk), stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_full=bool(se_full), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_se=d_se, d_y=d_y, d_fx=d_fx, d_keep=d_keep, d_sa_inv=d_sa_inv, d_cost=d_cost,
                      d_cost_obs=d_cost_obs, d_cost_prior=d_cost_prior, d_status=d_status, d_active=d_active))

    @_serialised
    def oe_nform_prepare_device(self, nprof, nlev, m, d_k, d_x, d_xa, d_se, d_y, d_fx, d_h, d_g, d_rwr, d_keep, d_nobs,
                                d_lin_status, d_active=None, xa_per_profile=False, se_per_profile=False, stream=None,
                                reserved=0, struct_size=None):
        """The n-form linearisation at x (include/mwrt.h mwrt_oe_nform_prepare_device), one pass over ``d_k``: writes
        ``d_h [nprof][n (n + 1) / 2]`` (K^T W K packed), ``d_g [nprof][n]``, ``d_rwr [nprof]``, ``d_keep [nprof][m]`` (uint8),
        ``d_nobs [nprof]`` (int32) and ``d_lin_status [nprof]`` (uint8).  ``d_se`` holds variances, ``[m]`` or, with
        ``se_per_profile``, ``[nprof][m]``; m is not bounded, n = nblk nlev is (``OE_NFORM_MAX_N``)."""
        self._oe(MwrtOeNform, "mwrt_oe_nform_prepare_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_per_profile=bool(se_per_profile), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_se=d_se, d_y=d_y, d_fx=d_fx, d_h=d_h, d_g=d_g, d_rwr=d_rwr, d_keep=d_keep,
                      d_nobs=d_nobs, d_lin_status=d_lin_status, d_active=d_active))

    @_serialised
    def oe_nform_solve_device(self, nprof, nlev, m, nblk, d_x, d_xa, d_sa_inv, d_h, d_g, d_rwr, d_lin_status, d_x_new,
                              d_status, d_gamma=None, d_chi2=None, d_dfs=None, d_post_var=None, d_post_cov=None,
                              d_active=None, xa_per_profile=False, stream=None, reserved=0, struct_size=None):
        """One step on an n-form linearisation (include/mwrt.h mwrt_oe_nform_solve_device), damped with ``d_gamma [nprof]``
        when it is given: ``d_x_new [nprof][nblk][nlev]`` and ``d_status [nprof]`` (uint8) required; ``d_chi2``, ``d_dfs``,
        ``d_post_var`` and ``d_post_cov [nprof][n][n]`` optional and defined without ``d_gamma`` only.  ``nblk`` is the number
        of state blocks (the call reads no K)."""
        self._oe(MwrtOeNform, "mwrt_oe_nform_solve_device", nprof, nlev, m, [None] * int(nblk), stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_sa_inv=d_sa_inv, d_h=d_h, d_g=d_g, d_rwr=d_rwr, d_lin_status=d_lin_status,
                      d_x_new=d_x_new, d_status=d_status, d_gamma=d_gamma, d_chi2=d_chi2, d_dfs=d_dfs, d_post_var=d_post_var,
                      d_post_cov=d_post_cov, d_active=d_active))

    @_serialised
    def oe_nform_cost_device(self, nprof, nlev, m, nblk, d_x, d_xa, d_sa_inv, d_se, d_y, d_fx, d_keep, d_cost,
                             d_cost_obs=None, d_cost_prior=None, d_status=None, d_active=None, xa_per_profile=False,
                             se_per_profile=False, stream=None, reserved=0, struct_size=None):
        """J = sum over the rows ``d_keep`` names of (y - fx)^2 / se + (x - xa)^T Sa^-1 (x - xa) (include/mwrt.h
        mwrt_oe_nform_cost_device); ``nblk`` is the number of state blocks (the call reads no K)."""
        self._oe(MwrtOeNform, "mwrt_oe_nform_cost_device", nprof, nlev, m, [None] * int(nblk), stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_per_profile=bool(se_per_profile), reserved=reserved),
                 dict(d_x=d_x, d_xa=d_xa, d_sa_inv=d_sa_inv, d_se=d_se, d_y=d_y, d_fx=d_fx, d_keep=d_keep, d_cost=d_cost,
                      d_cost_obs=d_cost_obs, d_cost_prior=d_cost_prior, d_status=d_status, d_active=d_active))

    @_serialised
    def oe_nform_char_device(self, nprof, nlev, m, nblk, d_sa_inv, d_h, d_lin_status, d_status, d_post_cov=None, d_avk=None,
                             d_avk_diag=None, d_dfs_block=None, d_noise_var=None, d_smooth_var=None, d_active=None,
                             row_begin=0, row_count=0, stream=None, reserved=0, struct_size=None):
        """The characterisation of the undamped n-form step on a linearisation (include/mwrt.h mwrt_oe_nform_char_device):
        ``d_h`` and ``d_lin_status`` as ``oe_nform_prepare_device`` wrote them and ``d_sa_inv [n][n]``; ``d_status [nprof]``
        (uint8) required and at least one of ``d_post_cov [nprof][n][n]``, ``d_avk [nprof][rows][n]`` (rows ``row_begin ..
        row_begin + row_count - 1``; ``row_count=0`` with ``row_begin=0``: all n), ``d_avk_diag`` / ``d_noise_var`` /
        ``d_smooth_var [nprof][nblk][nlev]`` and ``d_dfs_block [nprof][nblk]``.  ``nblk`` is the number of state blocks (the
        call reads no K)."""
        self._oe(MwrtOeNformChar, "mwrt_oe_nform_char_device", nprof, nlev, m, [None] * int(nblk), stream, struct_size,
                 dict(row_begin=row_begin, row_count=row_count, reserved=reserved),
                 dict(d_sa_inv=d_sa_inv, d_h=d_h, d_lin_status=d_lin_status, d_status=d_status, d_post_cov=d_post_cov,
                      d_avk=d_avk, d_avk_diag=d_avk_diag, d_dfs_block=d_dfs_block, d_noise_var=d_noise_var,
                      d_smooth_var=d_smooth_var, d_active=d_active))

    @_serialised
    def oe_nform_gain_device(self, nprof, nlev, m, d_k, d_se, d_keep, d_post_cov, d_status, d_gain, d_active=None,
                             se_per_profile=False, stream=None, reserved=0, struct_size=None):
        """The gain matrix of the undamped n-form step (include/mwrt.h mwrt_oe_nform_gain_device) into ``d_gain
        [nprof][m][n]``: row i is S^ k_i / se_i from the K blocks ``d_k``, the variances ``d_se`` (``[m]`` or, with
        ``se_per_profile``, ``[nprof][m]``) and ``d_keep`` as prepare saw and wrote them, and ``d_post_cov``, ``d_status`` as
        ``oe_nform_char_device`` (or ``oe_nform_solve_device`` without ``d_gamma``) wrote them."""
        self._oe(MwrtOeNformChar, "mwrt_oe_nform_gain_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(se_per_profile=bool(se_per_profile), reserved=reserved),
                 dict(d_se=d_se, d_keep=d_keep, d_post_cov=d_post_cov, d_status=d_status, d_gain=d_gain, d_active=d_active))

    @_serialised
    def oe_select_device(self, nprof, nlev, m, d_k, d_s0, d_se, nsel, d_order, d_q_pick, d_rank, d_q, d_count, d_status,
                         d_sa_inv=None, d_keep=None, d_candidate=None, d_active=None, d_dfs_gain=None, d_post_cov=None,
                         d_post_var=None, se_per_profile=False, s0_per_profile=False, stream=None, reserved=0,
                         struct_size=None):
        """Observation selection by information content (include/mwrt.h mwrt_oe_select_device): the greedy order of the
        ``nsel`` rows of the K blocks ``d_k`` that reduce the entropy of ``d_s0`` (``[n][n]`` or, with ``s0_per_profile``,
        ``[nprof][n][n]``) most, under the variances ``d_se`` (``[m]`` or, with ``se_per_profile``, ``[nprof][m]``).  Writes
        ``d_order`` (int32) and ``d_q_pick [nprof][nsel]``, ``d_rank`` (int32) and ``d_q [nprof][m]``, ``d_count`` (int32)
        and ``d_status [nprof]`` (uint8); optional ``d_dfs_gain [nprof][nsel]`` (needs ``d_sa_inv [n][n]``), ``d_post_cov
        [nprof][n][n]`` and ``d_post_var [nprof][nblk][nlev]``.  ``d_keep [nprof][m]``, ``d_candidate [m]`` and ``d_active
        [nprof]`` (uint8) narrow the candidates and the batch."""
        self._oe(MwrtOeSelect, "mwrt_oe_select_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(se_per_profile=bool(se_per_profile), s0_per_profile=bool(s0_per_profile), nsel=nsel, reserved=reserved),
                 dict(d_s0=d_s0, d_se=d_se, d_sa_inv=d_sa_inv, d_keep=d_keep, d_candidate=d_candidate, d_active=d_active,
                      d_order=d_order, d_q_pick=d_q_pick, d_rank=d_rank, d_q=d_q, d_count=d_count, d_status=d_status,
                      d_dfs_gain=d_dfs_gain, d_post_cov=d_post_cov, d_post_var=d_post_var))

    @_serialised
    def oe_gain_device(self, nprof, nlev, m, d_k, d_x, d_xa, d_sa, d_se, d_y, d_fx, d_status, d_gain=None, d_ksa=None,
                       d_keep=None, d_avk_diag=None, d_dfs_block=None, d_noise_var=None, d_smooth_var=None, d_nobs=None,
                       xa_per_profile=False, se_full=False, stream=None, reserved=0, reserved2=0, struct_size=None):
        """The gain matrix and the error budget of one step (include/mwrt.h mwrt_oe_gain_device): the inputs of
        ``oe_step_device``; ``d_status [nprof]`` (uint8) required, and at least one of ``d_gain`` and ``d_ksa``
        ``[nprof][m][n]``, ``d_keep [nprof][m]`` (uint8), ``d_avk_diag`` / ``d_noise_var`` / ``d_smooth_var``
        ``[nprof][nblk][nlev]``, ``d_dfs_block [nprof][nblk]`` and ``d_nobs [nprof]`` (int32)."""
        self._oe(MwrtOeChar, "mwrt_oe_gain_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(xa_per_profile=bool(xa_per_profile), se_full=bool(se_full), reserved=reserved, reserved2=reserved2),
                 dict(d_x=d_x, d_xa=d_xa, d_sa=d_sa, d_se=d_se, d_y=d_y, d_fx=d_fx, d_status=d_status, d_gain=d_gain,
                      d_ksa=d_ksa, d_keep=d_keep, d_avk_diag=d_avk_diag, d_dfs_block=d_dfs_block, d_noise_var=d_noise_var,
                      d_smooth_var=d_smooth_var, d_nobs=d_nobs))

    @_serialised
    def oe_product_device(self, nprof, nlev, m, product, d_gain, d_keep, d_out, d_k, d_ksa=None, d_sa=None, row_begin=0,
                          row_count=0, stream=None, reserved=0, reserved2=0, struct_size=None):
        """The averaging kernel (``OE_PRODUCT_AVK``: reads ``d_k``) or the posterior covariance (``OE_PRODUCT_POST_COV``:
        reads ``d_ksa`` and ``d_sa``; ``d_k`` then only tells the number of blocks and may hold None) from a gain entry's
        ``d_gain`` and ``d_keep`` (include/mwrt.h mwrt_oe_product_device), rows ``row_begin .. row_begin + row_count - 1``
        into ``d_out [nprof][row_count][n]``; ``row_count=0`` with ``row_begin=0`` is all n rows."""
        self._oe(MwrtOeChar, "mwrt_oe_product_device", nprof, nlev, m, d_k, stream, struct_size,
                 dict(product=product, row_begin=row_begin, row_count=row_count, reserved=reserved, reserved2=reserved2),
                 dict(d_gain=d_gain, d_keep=d_keep, d_out=d_out, d_ksa=d_ksa, d_sa=d_sa))

    @_serialised
    def obs_create(self, m_in, m_out, row_ptr, col, w) -> ctypes.c_void_p:
        """An instrument operator on this context (include/mwrt.h mwrt_obs_create) from the host CSR arrays ``row_ptr
        [m_out + 1]``, ``col [nnz]`` (int32) and ``w [nnz]`` (float64): checked and uploaded once.  Returns the handle
        ``obs_apply_device`` takes; release it with ``obs_destroy`` (before or after the context is closed)."""
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32).ravel()
        col = np.ascontiguousarray(col, dtype=np.int32).ravel()
        w = _f64(w).ravel()
        if row_ptr.size != int(m_out) + 1 or col.size != w.size or (row_ptr.size and row_ptr[-1] != w.size):
            raise ValueError(f"obs_create: expected row_ptr [{int(m_out) + 1}] ending at nnz = len(col) = len(w), got "
                             f"{row_ptr.size}, {col.size}, {w.size}")
        h = ctypes.c_void_p()
        self._check(self._lib.mwrt_obs_create(self._handle, int(m_in), int(m_out), _ptr(row_ptr), _ptr(col), _ptr(w),
                                              ctypes.byref(h)), "mwrt_obs_create")
        return h

    def obs_destroy(self, handle):
        """Releases an operator of ``obs_create`` (include/mwrt.h mwrt_obs_destroy); safe after ``close`` as well."""
        with self._lock:
            self._check(self._lib.mwrt_obs_destroy(handle), "mwrt_obs_destroy")

    @_serialised
    def obs_apply_device(self, handle, nprof, nlev, d_tb_in=None, d_tb_out=None, d_k_in=(), d_k_out=(), stream=None,
                         reserved=0, struct_size=None, nblk=None):
        """Applies an instrument operator (include/mwrt.h mwrt_obs_apply_device): ``d_tb_in [nprof][m_in]`` ->
        ``d_tb_out [nprof][m_out]`` (optional, as a pair) and, for each of up to four blocks, ``d_k_in[b]
        [nprof][m_in][nlev]`` -> ``d_k_out[b] [nprof][m_out][nlev]``.  ``nblk`` (default: ``len(d_k_in)``) and
        ``struct_size`` (default: the whole record) are what the record claims."""
        d_k_in = list(d_k_in)
        rec = _record(MwrtObsApply, struct_size, dict(nblk=len(d_k_in) if nblk is None else nblk, reserved=reserved),
                      dict(d_tb_in=d_tb_in, d_tb_out=d_tb_out), d_k_in=d_k_in, d_k_out=d_k_out)
        self._check(self._lib.mwrt_obs_apply_device(self._handle, handle, int(nprof), int(nlev), ctypes.byref(rec),
                                                    _stream(stream)), "mwrt_obs_apply_device")

    @_serialised
    def basis_create(self, nblk, nlev, b) -> ctypes.c_void_p:
        """A reduced basis on this context (include/mwrt.h mwrt_basis_create) from the host array ``b [nblk * nlev][r]``:
        checked and uploaded once.  Returns the handle ``basis_project_device`` and ``basis_expand_device`` take; release it
        with ``basis_destroy`` (before or after the context is closed)."""
        b = _f64(b)
        if b.ndim != 2 or b.shape[0] != int(nblk) * int(nlev):
            raise ValueError(f"basis_create: expected b [{int(nblk) * int(nlev)}][r], got {b.shape}")
        h = ctypes.c_void_p()
        self._check(self._lib.mwrt_basis_create(self._handle, int(nblk), int(nlev), b.shape[1], _ptr(b), ctypes.byref(h)),
                    "mwrt_basis_create")
        return h

    def basis_destroy(self, handle):
        """Releases a basis of ``basis_create`` (include/mwrt.h mwrt_basis_destroy); safe after ``close`` as well."""
        with self._lock:
            self._check(self._lib.mwrt_basis_destroy(handle), "mwrt_basis_destroy")

    @_serialised
    def basis_project_device(self, handle, nprof, m, d_k_in, d_k_out, stream=None, reserved=0, struct_size=None, reserved2=0):
        """K B (include/mwrt.h mwrt_basis_project_device): the blocks ``d_k_in[b] [nprof][m][nlev]`` of the basis' nblk ->
        ``d_k_out [nprof][m][r]``.  ``struct_size`` (default: the whole record) is what the record claims."""
        rec = _record(MwrtBasisApply, struct_size, dict(reserved=reserved, reserved2=reserved2), dict(d_k_out=d_k_out),
                      d_k_in=d_k_in)
        self._check(self._lib.mwrt_basis_project_device(self._handle, handle, int(nprof), int(m), ctypes.byref(rec),
                                                        _stream(stream)), "mwrt_basis_project_device")

    @_serialised
    def basis_expand_device(self, handle, nprof, d_c, d_x_ref, d_x, x_ref_per_profile=False, stream=None, reserved=0,
                            struct_size=None, reserved2=0):
        """x_ref + B c (include/mwrt.h mwrt_basis_expand_device): ``d_c [nprof][r]`` and ``d_x_ref [n]`` (``[nprof][n]``
        with ``x_ref_per_profile``) -> ``d_x [nprof][n]``."""
        rec = _record(MwrtBasisApply, struct_size,
                      dict(reserved=reserved, reserved2=reserved2, x_ref_per_profile=bool(x_ref_per_profile)),
                      dict(d_c=d_c, d_x_ref=d_x_ref, d_x=d_x))
        self._check(self._lib.mwrt_basis_expand_device(self._handle, handle, int(nprof), ctypes.byref(rec),
                                                       _stream(stream)), "mwrt_basis_expand_device")

    @staticmethod
    def _whiten_record(d_se, d_y, d_fx, d_k_in, d_l, d_keep, d_status, d_y_out, d_fx_out, d_k_out, se_full, mode, reserved,
                       struct_size, nblk):
        d_k_in = list(d_k_in)
        return _record(MwrtObsWhiten, struct_size,
                       dict(nblk=len(d_k_in) if nblk is None else nblk, se_full=bool(se_full), mode=mode, reserved=reserved),
                       dict(d_se=d_se, d_y=d_y, d_fx=d_fx, d_l=d_l, d_keep=d_keep, d_status=d_status, d_y_out=d_y_out,
                            d_fx_out=d_fx_out), d_k_in=d_k_in, d_k_out=d_k_out)

    @_serialised
    def obs_whiten_device(self, nprof, nlev, m, d_se, d_y, d_fx, d_k_in, d_l, d_keep, d_status, d_y_out=None, d_fx_out=None,
                          d_k_out=(), se_full=False, stream=None, mode=0, reserved=0, struct_size=None, nblk=None):
        """Pre-whitening with a per-profile Se (include/mwrt.h mwrt_obs_whiten_device): decides the rows each profile
        keeps, factorises the kept ``d_se [nprof][m]`` (``[nprof][m][m]`` with ``se_full``) into ``d_l [nprof][m (m + 1) / 2]``
        with ``d_keep [nprof][m]`` and ``d_status [nprof]`` (uint8), and writes L^-1 y, L^-1 F and L^-1 K_b into the outputs
        asked for (``None`` in ``d_k_out`` skips a block).  ``nblk`` (default: ``len(d_k_in)``) and ``struct_size``
        (default: the whole record) are what the record claims."""
        rec = self._whiten_record(d_se, d_y, d_fx, d_k_in, d_l, d_keep, d_status, d_y_out, d_fx_out, d_k_out, se_full, mode,
                                  reserved, struct_size, nblk)
        self._check(self._lib.mwrt_obs_whiten_device(self._handle, int(nprof), int(nlev), int(m), ctypes.byref(rec),
                                                     _stream(stream)), "mwrt_obs_whiten_device")

    @_serialised
    def obs_whiten_apply_device(self, nprof, nlev, m, d_l, d_keep, mode=0, d_y=None, d_y_out=None, d_fx=None, d_fx_out=None,
                                d_k_in=(), d_k_out=(), stream=None, reserved=0, struct_size=None, nblk=None):
        """Applies a stored factor (include/mwrt.h mwrt_obs_whiten_apply_device): ``mode`` 0 is L^-1, 1 is L^-T, on the
        vectors ``d_y -> d_y_out`` and ``d_fx -> d_fx_out`` ``[nprof][m]`` (each optional, as a pair) and on the blocks
        ``d_k_in[b] -> d_k_out[b] [nprof][m][nlev]``."""
        rec = self._whiten_record(None, d_y, d_fx, d_k_in, d_l, d_keep, None, d_y_out, d_fx_out, d_k_out, False, mode,
                                  reserved, struct_size, nblk)
        self._check(self._lib.mwrt_obs_whiten_apply_device(self._handle, int(nprof), int(nlev), int(m), ctypes.byref(rec),
                                                           _stream(stream)), "mwrt_obs_whiten_apply_device")

    def layer_tau_pitch(self, nf: int) -> int:
        """Doubles between consecutive levels of a layer-optical-depth array for nf frequencies (multiple of 16)."""
        return int(self._lib.mwrt_layer_tau_pitch(int(nf)))

    @_serialised
    def layer_tau_batch_device(self, model, nprof, nlev, d_z, d_p, d_t, d_rh, frq, d_tau, tau_pitch, d_valid, stream=None):
        """K1 + layer step: zenith layer optical depth [nprof][nlev][tau_pitch] (8 B per point) and valid [nprof]."""
        frq = _f64(frq).ravel()
        self._check(self._lib.mwrt_layer_tau_batch_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_z), _ptr(d_p), _ptr(d_t), _ptr(d_rh),
            frq.size, _ptr(frq), _ptr(d_tau), int(tau_pitch), _ptr(d_valid), _stream(stream)), "mwrt_layer_tau_batch_device")

    @_serialised
    def tb_from_layer_tau_device(self, model, nprof, nlev, d_tau, tau_pitch, d_t, frq, elev, d_valid, d_tb, stream=None):
        """K2: downwelling RTE from layer optical depths already in HBM (lane = frequency kernel)."""
        frq, elev = _f64(frq).ravel(), _f64(elev).ravel()
        self._check(self._lib.mwrt_tb_from_layer_tau_device(
            self._handle, self.model(model), int(nprof), int(nlev), _ptr(d_tau), int(tau_pitch), _ptr(d_t), frq.size,
            _ptr(frq), elev.size, _ptr(elev), _ptr(d_valid), _ptr(d_tb), _stream(stream)), "mwrt_tb_from_layer_tau_device")

    @_serialised
    def set_chunk_width(self, width: int):
        """Frequencies per workgroup of the fused TB kernel: 0 automatic, 8 / 14 / 16 (include/mwrt.h)."""
        self._check(self._lib.mwrt_set_chunk_width(self._handle, int(width)), "mwrt_set_chunk_width")

    def set_absorption_mode(self, mode: int):
        """0 automatic, 1 every line at every frequency, 2 windowed (fine grids; include/mwrt.h)."""
        self._check(self._lib.mwrt_set_absorption_mode(self._handle, int(mode)), "mwrt_set_absorption_mode")

    @_serialised
    def selftest_math(self, x, y_pos):
        """(fexp(x), flog(y), fdiv(x, y), fdiv1(x, y)) as evaluated by the device helpers."""
        x, y = _f64(x).ravel(), _f64(y_pos).ravel()
        outs = [np.empty_like(x) for _ in range(4)]
        self._check(self._lib.mwrt_selftest_math(self._handle, x.size, _ptr(x), _ptr(y), *[_ptr(o) for o in outs]),
                    "mwrt_selftest_math")
        return outs

    @_serialised
    def selftest_helpers(self, helper, inputs, block=256, n=None):
        """One device helper on host arrays (mwrt_selftest_helpers; ``helper``: a key of HELPERS or its number;
        ``inputs``: up to four equally long arrays).  Returns (four float64 output arrays, the uint8 flag array)."""
        helper = HELPERS[helper] if isinstance(helper, str) else int(helper)
        ins = [_f64(a).ravel() for a in inputs]
        n = (ins[0].size if ins else 0) if n is None else int(n)
        if n >= 0 and any(a.size != n for a in ins):
            raise ValueError("selftest_helpers: every input holds n elements")
        outs = [np.zeros(max(n, 0)) for _ in range(4)]
        flag = np.zeros(max(n, 0), dtype=np.uint8)
        ptrs = [_ptr(a) for a in ins] + [None] * (4 - len(ins))
        self._check(self._lib.mwrt_selftest_helpers(self._handle, helper, n, int(block), *ptrs, *[_ptr(o) for o in outs],
                                                    _ptr(flag)), "mwrt_selftest_helpers")
        return outs, flag

    @_serialised
    def synchronize(self, stream=None):
        self._check(self._lib.mwrt_synchronize(self._handle, _stream(stream)), "mwrt_synchronize")

    @_serialised
    def set_timing(self, enabled: bool):
        self._check(self._lib.mwrt_set_timing(self._handle, int(bool(enabled))), "mwrt_set_timing")

    @_serialised
    def timing_collect(self):
        """(total device ms, number of launches) since timing was enabled / last collected."""
        ms, n = ctypes.c_double(), ctypes.c_int32()
        self._check(self._lib.mwrt_timing_collect(self._handle, ctypes.byref(ms), ctypes.byref(n)), "mwrt_timing_collect")
        return ms.value, n.value

    @_serialised
    def last_kernel_ms(self) -> float:
        ms = ctypes.c_double()
        self._check(self._lib.mwrt_last_kernel_ms(self._handle, ctypes.byref(ms)), "mwrt_last_kernel_ms")
        return ms.value


_default_ctx: Dict[int, Context] = {}


def default_context(device_id: int = 0) -> Context:
    """Process-wide context per device (what the TbCloudRTE shim uses)."""
    ctx = _default_ctx.get(device_id)
    if ctx is None or ctx._handle is None:
        ctx = _default_ctx[device_id] = Context(device_id)
    return ctx
