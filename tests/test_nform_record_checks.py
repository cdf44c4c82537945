"""The argument stage of the n-form entries (csrc/mwrt_records.cpp oe_nform_args) without a GPU: tests/record_dump.cpp links
it as is, built with the host C++ compiler under ASan + UBSan and run as a child process (tests/record_kit.py: the fixture
and the helpers; the cut of the record at every struct_size is held with the other records' by tests/test_record_checks.py).
The record is built from the ctypes mirror of _native.py, so the mirror and the C struct are held against each other too.
Pointer fields hold small distinct integers; nothing dereferences them."""
import ctypes

import pytest

from mwr_fast_forward_operators_and_lbls_amd import _native
from record_kit import INVALID, OK, UNSUPPORTED, line, record, record_dump, run      # noqa: F401 (record_dump: the fixture)

CLS = _native.MwrtOeNform
MINIMUM = 24                                         # the fixed part (through reserved, with its padding)
MAX_N = 128                                          # MWRT_OE_NFORM_MAX_N
SIGNS = "nprof < 0, nlev < 1 or m < 1"
TOO_SMALL = "mwrt_oe_nform.struct_size too small for the fixed part (through reserved)"
NBLK = "mwrt_oe_nform.nblk must be 1 .. 4"
RESERVED = "mwrt_oe_nform.reserved must be 0"
GAMMA = "mwrt_oe_nform: d_chi2, d_dfs, d_post_var and d_post_cov are defined at gamma = 0 only (d_gamma must be NULL)"
N_LIMIT = "n = nblk * nlev > MWRT_OE_NFORM_MAX_N (128 state elements per profile: the packed triangle of C lives in LDS)"
#: entry -> (the pointers it requires, pointers it leaves optional)
ENTRIES = {
    "nform_prepare": ("d_x d_xa d_se d_y d_fx d_h d_g d_rwr d_keep d_nobs d_lin_status d_k_0", "d_sa_inv d_gamma d_x_new d_cost"),
    "nform_solve": ("d_x d_xa d_sa_inv d_h d_g d_rwr d_lin_status d_x_new d_status", "d_k_0 d_se d_y d_keep d_nobs d_gamma d_cost"),
    "nform_cost": ("d_x d_xa d_sa_inv d_se d_y d_fx d_keep d_cost", "d_k_0 d_h d_gamma d_status d_cost_obs d_x_new"),
}
DIAGNOSTICS = ("d_chi2", "d_dfs", "d_post_var", "d_post_cov")


def rec(gamma=False, **kw):
    """A record the three entries accept: every pointer given but d_gamma, which excludes the diagnostics."""
    return record(CLS, **dict({} if gamma else {"d_gamma": None}, **kw))


def test_the_mirror_is_the_record():
    assert ctypes.sizeof(CLS) == 240 and CLS.d_k.offset == MINIMUM and CLS.d_x.offset == 56 and CLS.d_cost_prior.offset == 232
    assert [name for name, _ in CLS._fields_[:5]] == ["struct_size", "nblk", "xa_per_profile", "se_per_profile", "reserved"]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_their_messages_and_their_order(record_dump, entry):
    required, optional = (s.split() for s in ENTRIES[entry])
    cases = [
        (line(entry, 3, 2, 3, rec()), OK, None, rec()),
        (line(entry, 0, 1, 1, rec(nblk=4)), OK, None),
        (line(entry, 1, 2, 3, rec(d_k_1=None, d_k_2=None, d_k_3=None)), OK, None),       # beyond nblk: not looked at
        (line(entry, 1, 2, 3, rec(xa_per_profile=1, se_per_profile=1)), OK, None),
        # the limit is on n = nblk nlev, not on m
        (line(entry, 1, MAX_N, 3, rec()), OK, None),
        (line(entry, 1, 32, 3, rec(nblk=4)), OK, None),
        (line(entry, 1, 2, 141, rec()), OK, None),
        (line(entry, 1, 2, 2 ** 31 - 1, rec()), OK, None),
        (line(entry, 1, MAX_N + 1, 3, rec()), UNSUPPORTED, N_LIMIT),
        (line(entry, 1, 65, 3, rec(nblk=2)), UNSUPPORTED, N_LIMIT),
        (line(entry, 1, 2 ** 31 - 1, 3, rec(nblk=4)), UNSUPPORTED, N_LIMIT),
        (line(entry, 2 ** 31, 2, 3, rec()), UNSUPPORTED, "nprof exceeds grid limit"),
        (line(entry, 1, 2, 3, rec(struct_size=MINIMUM - 1)), INVALID, TOO_SMALL),
        (line(entry, 1, 2, 3, rec(struct_size=0)), INVALID, TOO_SMALL),
        (line(entry, -1, 2, 3, rec()), INVALID, SIGNS),
        (line(entry, 1, 0, 3, rec()), INVALID, SIGNS),
        (line(entry, 1, 2, 0, rec()), INVALID, SIGNS),
        (line(entry, 1, 2, 3, rec(nblk=0)), INVALID, NBLK),
        (line(entry, 1, 2, 3, rec(nblk=5)), INVALID, NBLK),
        (line(entry, 1, 2, 3, rec(reserved=1)), INVALID, RESERVED),
        # two checks would fire: the earlier one is reported
        (line(entry, -1, 2, 3, rec(struct_size=MINIMUM - 1)), INVALID, TOO_SMALL),
        (line(entry, -1, 2, 3, rec(nblk=0)), INVALID, SIGNS),
        (line(entry, 1, 2, 3, rec(nblk=5, reserved=1)), INVALID, NBLK),
        (line(entry, 1, 2, 3, rec(reserved=1, **{required[0]: None})), INVALID, RESERVED),
        (line(entry, 1, MAX_N + 1, 3, rec(**{required[0]: None})), INVALID, "null buffer"),
        (line(entry, 2 ** 31, MAX_N + 1, 3, rec()), UNSUPPORTED, N_LIMIT),
        # the shortest record: no pointer is read
        (line(entry, 1, 2, 3, rec(struct_size=MINIMUM)), INVALID, "null buffer"),
    ]
    cases += [(line(entry, 1, 2, 3, rec(**{p: None})), INVALID, "null buffer") for p in required]
    cases += [(line(entry, 1, 2, 3, rec(**{p: None})), OK, None) for p in optional]
    if entry == "nform_prepare":
        cases.append((line(entry, 1, 2, 3, rec(nblk=2, d_k_1=None)), INVALID, "null buffer"))
    else:                                                                            # solve and cost read no K block
        cases.append((line(entry, 1, 2, 3, rec(nblk=2, d_k_0=None, d_k_1=None)), OK, None))
    none = {p: None for p in DIAGNOSTICS}
    if entry == "nform_solve":
        cases += [(line(entry, 1, 2, 3, rec(gamma=True, **dict(none, **{p: 0x40}))), INVALID, GAMMA) for p in DIAGNOSTICS]
        cases += [
            (line(entry, 1, 2, 3, rec(gamma=True, **none)), OK, None),
            (line(entry, 1, 2, 3, rec(**none)), OK, None),
            (line(entry, 1, 2, 3, rec(gamma=True, d_x=None)), INVALID, "null buffer"),               # the pointers come first
            (line(entry, 1, MAX_N + 1, 3, rec(gamma=True)), INVALID, GAMMA),                          # ... the limits last
            # a record that ends before d_chi2 (or inside it): the diagnostics read as NULL, so d_gamma may be given
            (line(entry, 1, 2, 3, rec(gamma=True, struct_size=CLS.d_chi2.offset + 7)), OK, None),
            (line(entry, 1, 2, 3, rec(gamma=True, struct_size=CLS.d_chi2.offset + 8)), INVALID, GAMMA),
            (line(entry, 1, 2, 3, rec(struct_size=CLS.d_status.offset + 7)), INVALID, "null buffer"),  # ends inside d_status
        ]
    else:                                                                            # d_gamma and the diagnostics: not looked at
        cases.append((line(entry, 1, 2, 3, rec(gamma=True)), OK, None))
    run(record_dump, cases)
