"""The argument stage of the record entries (csrc/mwrt_records.cpp) without a GPU: tests/record_dump.cpp links it as is,
built with the host C++ compiler under ASan + UBSan and run as a child process (tests/record_kit.py: the fixture and the
helpers).  The cut of all nine records is held here; the entries of the three newest have modules of their own.  The
records are built from the ctypes mirrors of _native.py, so the mirrors and the C structs are held against each other too.
Pointer fields hold small distinct integers; nothing dereferences them."""
import ctypes

import pytest

from mwr_fast_forward_operators_and_lbls_amd import _native
from record_kit import INVALID, OK, UNSUPPORTED, leaves, line, put, record, record_dump, run      # noqa: F401 (the fixture)

MAX_LEVELS, MAX_M = 1024, 140                        # MWRT_MAX_LEVELS, MWRT_OE_MAX_M

#: record -> (ctypes mirror, documented minimum struct_size: include/mwrt.h)
RECORDS = {
    "mwrt_oe_step": (_native.MwrtOeStep, _native.MwrtOeStep.d_status.offset + 8),      # through d_status
    "mwrt_oe_lm": (_native.MwrtOeLm, 24),
    "mwrt_oe_char": (_native.MwrtOeChar, 24),
    "mwrt_obs_apply": (_native.MwrtObsApply, 12),
    "mwrt_basis_apply": (_native.MwrtBasisApply, 8),
    "mwrt_obs_whiten": (_native.MwrtObsWhiten, 24),
    "mwrt_oe_nform": (_native.MwrtOeNform, 24),      # these three: the fixed part (through reserved, with its padding)
    "mwrt_oe_nform_char": (_native.MwrtOeNformChar, 24),
    "mwrt_oe_select": (_native.MwrtOeSelect, 24),
}
#: sizeof + 9 requests each: struct_size 0 .. sizeof + 8
CUT_REQUESTS = {"mwrt_oe_step": 161, "mwrt_oe_lm": 233, "mwrt_oe_char": 209, "mwrt_obs_apply": 105, "mwrt_basis_apply": 89,
                "mwrt_obs_whiten": 161, "mwrt_oe_nform": 249, "mwrt_oe_nform_char": 177, "mwrt_oe_select": 185}


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_the_cut_at_every_struct_size(record_dump, name):
    """The record at every struct_size from 0 to sizeof + 8 with every field non-zero: below the documented minimum it is
    refused; from there on a field comes through if and only if it lies wholly below min(struct_size, sizeof), every other
    byte is zero (a field beyond the cut reads as NULL / 0).  The expectation is built from the ctypes offsets and sizes.
    The child owns exactly struct_size bytes."""
    cls, minimum = RECORDS[name]
    size = ctypes.sizeof(cls)
    rec = cls()
    for k, (field, index, _, width) in enumerate(leaves(cls)):
        put(rec, field, index, (k + 1) * 0x0101 + (0x01010000 << 8 if width == 8 else 0))
    full = bytes(rec) + b"\xab" * 8
    assert all(full[off:off + width].count(0) < width for _, _, off, width in leaves(cls))
    asked, want = [], []
    for struct_size in range(size + 9):
        caller = struct_size.to_bytes(4, "little") + full[4:max(struct_size, 4)]
        asked.append(f"cut {name} {caller.hex()}")
        expect = bytearray(size)
        for _, _, off, width in leaves(cls):
            if struct_size >= minimum and off + width <= min(struct_size, size):
                expect[off:off + width] = caller[off:off + width]
        want.append((struct_size, OK if struct_size >= minimum else INVALID, bytes(expect).hex()))
    assert len(asked) == CUT_REQUESTS[name] == size + 9 and sorted(CUT_REQUESTS) == sorted(RECORDS)
    for (struct_size, status, expect), got in zip(want, record_dump(asked)):
        assert (got["status"], got["record"]) == (status, expect), struct_size


NLEV_LIMIT = "nlev > MWRT_MAX_LEVELS (1024)"
OE_M_LIMIT = "m > MWRT_OE_MAX_M (140 observations per profile: G lives in LDS)"
SIGNS = "nprof < 0, nlev < 1 or m < 1"
#: entry -> (record name, mirror, the pointers it requires beside the first nblk of d_k, a pointer it leaves optional)
OE_ENTRIES = {
    "oe_step": ("mwrt_oe_step", _native.MwrtOeStep, "d_x d_xa d_sa d_se d_y d_fx d_x_new d_status d_k_0", "d_chi2"),
    "oe_lm_prepare": ("mwrt_oe_lm", _native.MwrtOeLm,
                      "d_x d_xa d_sa d_se d_y d_fx d_g0 d_r d_kdx d_keep d_lin_status d_k_0", "d_gamma"),
    "oe_lm_solve": ("mwrt_oe_lm", _native.MwrtOeLm,
                    "d_x d_xa d_sa d_se d_gamma d_g0 d_r d_kdx d_keep d_lin_status d_x_new d_status d_k_0", "d_y"),
    "oe_cost": ("mwrt_oe_lm", _native.MwrtOeLm, "d_x d_xa d_se d_y d_fx d_keep d_sa_inv d_cost", "d_k_0"),
    "oe_gain": ("mwrt_oe_char", _native.MwrtOeChar, "d_x d_xa d_sa d_se d_y d_fx d_status d_k_0", "d_gain"),
    "oe_product": ("mwrt_oe_char", _native.MwrtOeChar, "d_gain d_keep d_out d_k_0", "d_x"),
}


@pytest.mark.parametrize("entry", sorted(OE_ENTRIES))
def test_the_optimal_estimation_entries(record_dump, entry):
    name, cls, required, optional = OE_ENTRIES[entry]
    required = required.split()
    what = "the required fields (through d_status)" if entry == "oe_step" else "the fixed part (through reserved)"
    too_small = f"{name}.struct_size too small for {what}"
    reserved = f"{name}.reserved and reserved2 must be 0" if cls is _native.MwrtOeChar else f"{name}.reserved must be 0"
    minimum = RECORDS[name][1]
    r = lambda **kw: record(cls, **kw)                                               # noqa: E731
    cases = [
        (line(entry, 3, 2, 3, r()), OK, None, r()),
        (line(entry, 0, 1, 1, r(nblk=4)), OK, None),
        (line(entry, 1, MAX_LEVELS, MAX_M, r(**{optional: None})), OK, None),
        (line(entry, 1, 2, 3, r(d_k_1=None, d_k_2=None, d_k_3=None)), OK, None),         # beyond nblk: not looked at
        (line(entry, 1, 2, 3, r(struct_size=minimum - 1)), INVALID, too_small),
        (line(entry, 1, 2, 3, r(struct_size=0)), INVALID, too_small),
        (line(entry, -1, 2, 3, r()), INVALID, SIGNS),
        (line(entry, 1, 0, 3, r()), INVALID, SIGNS),
        (line(entry, 1, 2, 0, r()), INVALID, SIGNS),
        (line(entry, 1, 2, 3, r(nblk=0)), INVALID, f"{name}.nblk must be 1 .. 4"),
        (line(entry, 1, 2, 3, r(nblk=5)), INVALID, f"{name}.nblk must be 1 .. 4"),
        (line(entry, 1, 2, 3, r(reserved=1)), INVALID, reserved),
        (line(entry, 1, MAX_LEVELS + 1, 3, r()), UNSUPPORTED, NLEV_LIMIT),
        (line(entry, 1, 2, MAX_M + 1, r()), UNSUPPORTED, OE_M_LIMIT),
        (line(entry, 2 ** 31, 2, 3, r()), UNSUPPORTED, "nprof exceeds grid limit"),
        # two checks would fire: the earlier one is reported
        (line(entry, -1, 2, 3, r(struct_size=minimum - 1)), INVALID, too_small),
        (line(entry, -1, 2, 3, r(nblk=0)), INVALID, SIGNS),
        (line(entry, 1, 2, 3, r(nblk=5, reserved=1)), INVALID, f"{name}.nblk must be 1 .. 4"),
        (line(entry, 1, 2, 3, r(reserved=1, **{required[0]: None})), INVALID, reserved),
        (line(entry, 1, MAX_LEVELS + 1, 3, r(**{required[0]: None})), INVALID, "null buffer"),
        (line(entry, 1, MAX_LEVELS + 1, MAX_M + 1, r()), UNSUPPORTED, NLEV_LIMIT),
        (line(entry, 2 ** 31, 2, MAX_M + 1, r()), UNSUPPORTED, OE_M_LIMIT),
    ]
    cases += [(line(entry, 1, 2, 3, r(**{p: None})), INVALID, "null buffer") for p in required]
    if entry != "oe_cost":                                                           # the cost reads no K block
        cases.append((line(entry, 1, 2, 3, r(nblk=2, d_k_1=None)), INVALID, "null buffer"))
    if cls is _native.MwrtOeChar:
        cases.append((line(entry, 1, 2, 3, r(reserved2=1)), INVALID, reserved))
    if entry == "oe_step":                   # the shortest record served: the optional outputs come out NULL
        short = r(struct_size=minimum, d_chi2=None, d_dfs=None, d_post_var=None, d_nobs=None)
        cases.append((line(entry, 1, 2, 3, r(struct_size=minimum)), OK, None, short))
    if entry == "oe_gain":
        outputs = "d_gain d_ksa d_keep d_avk_diag d_dfs_block d_noise_var d_smooth_var d_nobs".split()
        none = {p: None for p in outputs}
        no_output = "mwrt_oe_gain_device: no output asked for beside d_status"
        cases += [(line(entry, 1, 2, 3, r(**none)), INVALID, no_output),
                  (line(entry, 1, 2, 3, r(d_x=None, **none)), INVALID, "null buffer"),
                  (line(entry, 1, MAX_LEVELS + 1, 3, r(**none)), INVALID, no_output)]
        cases += [(line(entry, 1, 2, 3, r(**{p: None for p in outputs if p != keep})), OK, None) for keep in outputs]
        cases.append((line(entry, 1, 2, 3, r(product=7, row_begin=-1)), OK, None))      # the product's fields: not looked at
    if entry == "oe_product":
        product = "mwrt_oe_char.product must be MWRT_OE_PRODUCT_AVK or MWRT_OE_PRODUCT_POST_COV"
        rows = "mwrt_oe_char: rows row_begin .. row_begin + row_count - 1 must lie in 0 .. n - 1 (row_count 0 with row_begin 0: all rows)"
        cases += [
            (line(entry, 1, 2, 3, r(product=1, d_k_0=None)), OK, None),                  # S^ reads d_ksa and d_sa, no K
            (line(entry, 1, 2, 3, r(product=1, d_ksa=None)), INVALID, "null buffer"),
            (line(entry, 1, 2, 3, r(product=1, d_sa=None)), INVALID, "null buffer"),
            (line(entry, 1, 2, 3, r(d_ksa=None, d_sa=None)), OK, None),
            (line(entry, 1, 2, 3, r(product=2)), INVALID, product),
            (line(entry, 1, 2, 3, r(product=-1)), INVALID, product),
            (line(entry, 1, 2, 3, r(row_begin=1, row_count=1)), OK, None),
            (line(entry, 1, 2, 3, r(nblk=2, row_begin=0, row_count=4)), OK, None),
            (line(entry, 1, 2, 3, r(row_begin=-1, row_count=1)), INVALID, rows),
            (line(entry, 1, 2, 3, r(row_count=-1)), INVALID, rows),
            (line(entry, 1, 2, 3, r(row_begin=1, row_count=0)), INVALID, rows),
            (line(entry, 1, 2, 3, r(row_begin=1, row_count=2)), INVALID, rows),
            (line(entry, 1, 2, 3, r(row_begin=2 ** 31 - 1, row_count=2 ** 31 - 1)), INVALID, rows),
            (line(entry, 1, 2, 3, r(product=2, d_out=None)), INVALID, product),
            (line(entry, 1, 2, 3, r(reserved2=1, product=2)), INVALID, reserved),
            (line(entry, 1, 2, 3, r(d_out=None, row_count=-1)), INVALID, "null buffer"),
            (line(entry, 1, MAX_LEVELS + 1, 3, r(row_count=-1)), INVALID, rows),
            # a record that ends before `product`: AVK of all rows, and d_out reads as NULL; one that ends inside d_out
            (line(entry, 1, 2, 3, r(struct_size=cls.product.offset, product=2, row_begin=-1)), INVALID, "null buffer"),
            (line(entry, 1, 2, 3, r(struct_size=ctypes.sizeof(cls) - 1)), INVALID, "null buffer"),
        ]
    run(record_dump, cases)


def test_the_instrument_operator_entry(record_dump):
    cls = _native.MwrtObsApply
    r = lambda **kw: record(cls, **kw)                                               # noqa: E731
    no_tb = dict(d_tb_in=None, d_tb_out=None)
    nblk = "mwrt_obs_apply.nblk must be 0 .. 4"
    pair = "mwrt_obs_apply: d_tb_in and d_tb_out are given together or not at all"
    null = "mwrt_obs_apply: null pointer among the first nblk of d_k_in / d_k_out"
    aliased = "mwrt_obs_apply: an output pointer equals its input (the map is not applied in place)"
    too_small = "mwrt_obs_apply.struct_size too small for the fixed part (through reserved)"
    run(record_dump, [
        (line("obs_apply", 3, 2, r()), OK, None, r()),
        (line("obs_apply", 0, 1, r(nblk=4)), OK, None),
        (line("obs_apply", 1, MAX_LEVELS, r(nblk=0)), OK, None),
        (line("obs_apply", 1, 2, r(**no_tb)), OK, None),
        (line("obs_apply", 2 ** 31, 2, r()), OK, None),                                  # its limit is the launch geometry's
        (line("obs_apply", 1, 2, r(nblk=2, d_k_in_2=None, d_k_out_3=None)), OK, None),
        (line("obs_apply", 1, 2, r(struct_size=11)), INVALID, too_small),
        (line("obs_apply", -1, 2, r()), INVALID, "nprof < 0 or nlev < 1"),
        (line("obs_apply", 1, 0, r()), INVALID, "nprof < 0 or nlev < 1"),
        (line("obs_apply", 1, 2, r(nblk=-1)), INVALID, nblk),
        (line("obs_apply", 1, 2, r(nblk=5)), INVALID, nblk),
        (line("obs_apply", 1, 2, r(reserved=1)), INVALID, "mwrt_obs_apply.reserved must be 0"),
        (line("obs_apply", 1, 2, r(d_tb_out=None)), INVALID, pair),
        (line("obs_apply", 1, 2, r(d_tb_in=None)), INVALID, pair),
        (line("obs_apply", 1, 2, r(d_k_in_0=None)), INVALID, null),
        (line("obs_apply", 1, 2, r(nblk=2, d_k_out_1=None)), INVALID, null),
        (line("obs_apply", 1, 2, r(nblk=0, **no_tb)), INVALID, "mwrt_obs_apply: nothing to do (no TB pair and nblk = 0)"),
        (line("obs_apply", 1, 2, r(d_tb_in=0x40, d_tb_out=0x40)), INVALID, aliased),
        (line("obs_apply", 1, 2, r(nblk=2, d_k_in_1=0x40, d_k_out_1=0x40)), INVALID, aliased),
        (line("obs_apply", 1, MAX_LEVELS + 1, r()), UNSUPPORTED, NLEV_LIMIT),
        # two checks would fire: the earlier one is reported
        (line("obs_apply", -1, 2, r(struct_size=11)), INVALID, too_small),
        (line("obs_apply", 1, 0, r(nblk=5)), INVALID, "nprof < 0 or nlev < 1"),
        (line("obs_apply", 1, 2, r(nblk=5, reserved=1)), INVALID, nblk),
        (line("obs_apply", 1, 2, r(reserved=1, d_tb_in=None)), INVALID, "mwrt_obs_apply.reserved must be 0"),
        (line("obs_apply", 1, 2, r(d_tb_in=None, d_k_in_0=None)), INVALID, pair),
        (line("obs_apply", 1, 2, r(d_k_out_0=None, d_tb_in=0x40, d_tb_out=0x40)), INVALID, null),
        (line("obs_apply", 1, MAX_LEVELS + 1, r(d_tb_in=0x40, d_tb_out=0x40)), INVALID, aliased),
        # the shortest record: no pointer is read; one that ends inside d_tb_out: half a pair
        (line("obs_apply", 1, 2, r(struct_size=12)), INVALID, null),
        (line("obs_apply", 1, 2, r(struct_size=12, nblk=0)), INVALID, "mwrt_obs_apply: nothing to do (no TB pair and nblk = 0)"),
        (line("obs_apply", 1, 2, r(struct_size=cls.d_tb_out.offset + 7, nblk=0)), INVALID, pair),
    ])


def test_the_reduced_basis_entries(record_dump):
    cls = _native.MwrtBasisApply
    r = lambda **kw: record(cls, **kw)                                               # noqa: E731
    too_small = "mwrt_basis_apply.struct_size too small for the fixed part (through reserved)"
    reserved = "mwrt_basis_apply.reserved and reserved2 must be 0"
    null_in = "mwrt_basis_apply: null pointer among the first nblk of d_k_in"
    in_place = "mwrt_basis_apply: d_k_out equals one of its inputs (the product is not formed in place)"
    null_x = "mwrt_basis_apply: d_c, d_x_ref or d_x is null"
    x_in_place = "mwrt_basis_apply: d_x equals one of its inputs (the map is not applied in place)"
    project = lambda nblk, nprof, m, rec: line("basis_project", nblk, nprof, m, rec)      # noqa: E731
    run(record_dump, [
        (project(2, 3, 2, r()), OK, None, r()),
        (project(4, 0, 1, r()), OK, None),
        (project(2, 2 ** 31, 3, r(d_k_in_2=None, d_k_in_3=None, d_c=None, d_x_ref=None, d_x=None)), OK, None),
        (project(2, 1, 3, r(x_ref_per_profile=1)), OK, None),
        (project(2, 1, 3, r(struct_size=7)), INVALID, too_small),
        (project(2, -1, 3, r()), INVALID, "nprof < 0"),
        (project(2, 1, 3, r(reserved=1)), INVALID, reserved),
        (project(2, 1, 3, r(reserved2=1)), INVALID, reserved),
        (project(2, 1, 0, r()), INVALID, "m < 1"),
        (project(2, 1, 3, r(d_k_in_1=None)), INVALID, null_in),
        (project(2, 1, 3, r(d_k_out=None)), INVALID, "mwrt_basis_apply: d_k_out is null"),
        (project(2, 1, 3, r(d_k_in_1=0x40, d_k_out=0x40)), INVALID, in_place),
        (project(1, 1, 3, r(d_k_in_1=0x40, d_k_out=0x40)), OK, None),                      # beyond the basis' blocks
        # two checks would fire: the earlier one is reported
        (project(2, -1, 3, r(struct_size=7)), INVALID, too_small),
        (project(2, -1, 3, r(reserved=1)), INVALID, "nprof < 0"),
        (project(2, 1, 0, r(reserved2=1)), INVALID, reserved),
        (project(2, 1, 0, r(d_k_in_0=None)), INVALID, "m < 1"),
        (project(2, 1, 3, r(d_k_in_0=None, d_k_out=None)), INVALID, null_in),
        # a record that ends before reserved2 (or inside it): it is not read; the shortest record: no pointer is
        (project(2, 1, 3, r(struct_size=cls.reserved2.offset + 3, reserved2=1)), OK, None),
        (project(2, 1, 3, r(struct_size=8)), INVALID, null_in),
        (project(2, 1, 3, r(struct_size=cls.d_k_out.offset + 7)), INVALID, "mwrt_basis_apply: d_k_out is null"),
        (line("basis_expand", 3, r()), OK, None, r()),
        (line("basis_expand", 0, r(x_ref_per_profile=1, d_k_in_0=None, d_k_out=None)), OK, None),
        (line("basis_expand", 2 ** 31, r()), OK, None),
        (line("basis_expand", 1, r(struct_size=4)), INVALID, too_small),
        (line("basis_expand", -1, r()), INVALID, "nprof < 0"),
        (line("basis_expand", 1, r(reserved=1)), INVALID, reserved),
        (line("basis_expand", 1, r(reserved2=1)), INVALID, reserved),
        (line("basis_expand", 1, r(d_c=None)), INVALID, null_x),
        (line("basis_expand", 1, r(d_x_ref=None)), INVALID, null_x),
        (line("basis_expand", 1, r(d_x=None)), INVALID, null_x),
        (line("basis_expand", 1, r(d_c=0x40, d_x=0x40)), INVALID, x_in_place),
        (line("basis_expand", 1, r(d_x_ref=0x40, d_x=0x40)), INVALID, x_in_place),
        (line("basis_expand", -1, r(reserved2=1)), INVALID, "nprof < 0"),
        (line("basis_expand", 1, r(reserved=1, d_c=None)), INVALID, reserved),
        (line("basis_expand", 1, r(d_c=None, d_x_ref=0x40, d_x=0x40)), INVALID, null_x),
        (line("basis_expand", 1, r(struct_size=cls.d_x.offset + 4)), INVALID, null_x),
    ])


def test_the_pre_whitening_entries(record_dump):
    cls = _native.MwrtObsWhiten
    r = lambda **kw: record(cls, **kw)                                               # noqa: E731
    too_small = "mwrt_obs_whiten.struct_size too small for the fixed part (through reserved)"
    nblk = "mwrt_obs_whiten.nblk must be 0 .. 4"
    reserved = "mwrt_obs_whiten.reserved must be 0"
    mode_0 = "mwrt_obs_whiten.mode must be 0 in mwrt_obs_whiten_device"
    mode_01 = "mwrt_obs_whiten.mode must be 0 (L^-1) or 1 (L^-T)"
    null = "mwrt_obs_whiten: d_se, d_y, d_fx, d_l, d_keep or d_status is null"
    null_in = "mwrt_obs_whiten: null pointer among the first nblk of d_k_in"
    whitened_in_place = "mwrt_obs_whiten: an output pointer equals an input (nothing is whitened in place)"
    m_limit = "m > MWRT_OE_MAX_M (140)"
    cases = [
        (line("whiten", 3, 2, 3, r()), OK, None, r()),
        (line("whiten", 0, 1, 1, r(nblk=4, se_full=1)), OK, None),
        (line("whiten", 2 ** 31, MAX_LEVELS, MAX_M, r(nblk=0, d_k_in_0=None)), OK, None),
        (line("whiten", 1, 2, 3, r(d_y_out=None, d_fx_out=None, d_k_out_0=None, d_k_in_1=None)), OK, None),
        (line("whiten", 1, 2, 3, r(struct_size=cls.d_status.offset + 8)), OK, None,
         r(struct_size=cls.d_status.offset + 8, d_y_out=None, d_fx_out=None, d_k_out_0=None, d_k_out_1=None, d_k_out_2=None,
           d_k_out_3=None)),
        (line("whiten", 1, 2, 3, r(struct_size=23)), INVALID, too_small),
        (line("whiten", -1, 2, 3, r()), INVALID, SIGNS),
        (line("whiten", 1, 0, 3, r()), INVALID, SIGNS),
        (line("whiten", 1, 2, 0, r()), INVALID, SIGNS),
        (line("whiten", 1, 2, 3, r(nblk=-1)), INVALID, nblk),
        (line("whiten", 1, 2, 3, r(nblk=5)), INVALID, nblk),
        (line("whiten", 1, 2, 3, r(reserved=1 << 40)), INVALID, reserved),
        (line("whiten", 1, 2, 3, r(mode=1)), INVALID, mode_0),
        (line("whiten", 1, 2, 3, r(mode=-1)), INVALID, mode_0),
        (line("whiten", 1, 2, 3, r(d_k_in_0=None)), INVALID, null_in),
        (line("whiten", 1, 2, 3, r(nblk=2, d_k_in_1=None)), INVALID, null_in),
        (line("whiten", 1, 2, 3, r(d_y=0x40, d_y_out=0x40)), INVALID, whitened_in_place),
        (line("whiten", 1, 2, 3, r(d_se=0x40, d_l=0x40)), INVALID, whitened_in_place),
        (line("whiten", 1, 2, 3, r(d_k_in_0=0x40, d_k_out_3=0x40)), INVALID, whitened_in_place),
        (line("whiten", 1, 2, MAX_M + 1, r()), UNSUPPORTED, m_limit),
        (line("whiten", 1, MAX_LEVELS + 1, 3, r()), UNSUPPORTED, NLEV_LIMIT),
        # two checks would fire: the earlier one is reported
        (line("whiten", 1, 0, 3, r(struct_size=23)), INVALID, too_small),
        (line("whiten", 1, 2, 0, r(nblk=5)), INVALID, SIGNS),
        (line("whiten", 1, 2, 3, r(nblk=5, reserved=1)), INVALID, nblk),
        (line("whiten", 1, 2, 3, r(reserved=1, mode=1)), INVALID, reserved),
        (line("whiten", 1, 2, 3, r(mode=1, d_se=None)), INVALID, mode_0),
        (line("whiten", 1, 2, 3, r(d_se=None, d_k_in_0=None)), INVALID, null),
        (line("whiten", 1, 2, 3, r(d_k_in_0=None, d_y=0x40, d_y_out=0x40)), INVALID, null_in),
        (line("whiten", 1, 2, MAX_M + 1, r(d_y=0x40, d_y_out=0x40)), INVALID, whitened_in_place),
        (line("whiten", 1, MAX_LEVELS + 1, MAX_M + 1, r()), UNSUPPORTED, m_limit),
        (line("whiten", 1, 2, 3, r(struct_size=cls.d_status.offset + 7)), INVALID, null),      # ends inside d_status
    ]
    cases += [(line("whiten", 1, 2, 3, r(**{p: None})), INVALID, null) for p in "d_se d_y d_fx d_l d_keep d_status".split()]

    null = "mwrt_obs_whiten: d_l or d_keep is null"
    pair = "mwrt_obs_whiten: d_y and d_y_out (d_fx and d_fx_out) are given together or not at all"
    null_k = "mwrt_obs_whiten: null pointer among the first nblk of d_k_in / d_k_out"
    nothing = "mwrt_obs_whiten: nothing to do (no vector and nblk = 0)"
    applied_in_place = "mwrt_obs_whiten: an output pointer equals an input (nothing is applied in place)"
    no_vectors = dict(d_y=None, d_y_out=None, d_fx=None, d_fx_out=None)
    cases += [
        (line("whiten_apply", 3, 2, 3, r()), OK, None, r()),
        (line("whiten_apply", 0, 1, 1, r(nblk=4, mode=1)), OK, None),
        (line("whiten_apply", 1, MAX_LEVELS, MAX_M, r(d_se=None, d_status=None, **no_vectors)), OK, None),
        (line("whiten_apply", 1, 2, 3, r(nblk=0, d_fx=None, d_fx_out=None)), OK, None),
        (line("whiten_apply", 1, 2, 3, r(struct_size=16)), INVALID, too_small),
        (line("whiten_apply", -1, 2, 3, r()), INVALID, SIGNS),
        (line("whiten_apply", 1, 2, 3, r(nblk=5)), INVALID, nblk),
        (line("whiten_apply", 1, 2, 3, r(reserved=-1)), INVALID, reserved),
        (line("whiten_apply", 1, 2, 3, r(mode=2)), INVALID, mode_01),
        (line("whiten_apply", 1, 2, 3, r(mode=-1)), INVALID, mode_01),
        (line("whiten_apply", 1, 2, 3, r(d_l=None)), INVALID, null),
        (line("whiten_apply", 1, 2, 3, r(d_keep=None)), INVALID, null),
        (line("whiten_apply", 1, 2, 3, r(d_y_out=None)), INVALID, pair),
        (line("whiten_apply", 1, 2, 3, r(d_fx=None)), INVALID, pair),
        (line("whiten_apply", 1, 2, 3, r(d_k_in_0=None)), INVALID, null_k),
        (line("whiten_apply", 1, 2, 3, r(nblk=2, d_k_out_1=None)), INVALID, null_k),
        (line("whiten_apply", 1, 2, 3, r(nblk=0, **no_vectors)), INVALID, nothing),
        (line("whiten_apply", 1, 2, 3, r(d_k_in_0=0x40, d_k_out_0=0x40)), INVALID, applied_in_place),
        (line("whiten_apply", 1, 2, 3, r(d_l=0x40, d_y_out=0x40)), INVALID, applied_in_place),     # d_l is an input here
        (line("whiten_apply", 1, 2, MAX_M + 1, r()), UNSUPPORTED, m_limit),
        (line("whiten_apply", 1, MAX_LEVELS + 1, 3, r()), UNSUPPORTED, NLEV_LIMIT),
        # two checks would fire: the earlier one is reported
        (line("whiten_apply", 1, 2, 3, r(reserved=1, mode=2)), INVALID, reserved),
        (line("whiten_apply", 1, 2, 3, r(mode=2, d_l=None)), INVALID, mode_01),
        (line("whiten_apply", 1, 2, 3, r(d_l=None, d_y=None)), INVALID, null),
        (line("whiten_apply", 1, 2, 3, r(d_y=None, d_k_in_0=None)), INVALID, pair),
        (line("whiten_apply", 1, 2, 3, r(d_k_out_0=None, d_y=0x40, d_y_out=0x40)), INVALID, null_k),
        (line("whiten_apply", 1, MAX_LEVELS + 1, 3, r(d_y=0x40, d_y_out=0x40)), INVALID, applied_in_place),
        (line("whiten_apply", 1, MAX_LEVELS + 1, MAX_M + 1, r()), UNSUPPORTED, m_limit),
        (line("whiten_apply", 1, 2, 3, r(struct_size=cls.d_y_out.offset)), INVALID, pair),       # the outputs read as NULL
    ]
    run(record_dump, cases)
