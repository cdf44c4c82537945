"""The argument stage of the observation selection (csrc/mwrt_records.cpp oe_select_args) without a GPU:
tests/record_dump.cpp links it as is, built with the host C++ compiler under ASan + UBSan and run as a child process
(tests/record_kit.py: the fixture and the helpers; the cut of the record at every struct_size is held with the other
records' by tests/test_record_checks.py).  The record is built from the ctypes mirror of _native.py, so the mirror and the C
struct are held against each other too.  Pointer fields hold small distinct integers; nothing dereferences them."""
import ctypes

from mwr_fast_forward_operators_and_lbls_amd import _native
from record_kit import INVALID, OK, UNSUPPORTED, line, record, record_dump, run      # noqa: F401 (record_dump: the fixture)

CLS = _native.MwrtOeSelect
MINIMUM = 24                                         # the fixed part (through reserved)
MAX_N = 128                                          # MWRT_OE_NFORM_MAX_N
SIGNS = "nprof < 0, nlev < 1 or m < 1"
TOO_SMALL = "mwrt_oe_select.struct_size too small for the fixed part (through reserved)"
NBLK = "mwrt_oe_select.nblk must be 1 .. 4"
RESERVED = "mwrt_oe_select.reserved must be 0"
NSEL = "mwrt_oe_select.nsel must be 1 .. m"
DFS = "mwrt_oe_select: d_dfs_gain needs d_sa_inv (the degrees of freedom are taken against the prior)"
ALIASED = "mwrt_oe_select: an output pointer equals an input (nothing is formed in place)"
N_LIMIT = "n = nblk * nlev > MWRT_OE_NFORM_MAX_N (128 state elements per profile: the packed triangle of S lives in LDS)"
REQUIRED = "d_k_0 d_s0 d_se d_order d_q_pick d_rank d_q d_count d_status".split()
OPTIONAL = "d_keep d_candidate d_active d_dfs_gain d_post_cov d_post_var".split()
INPUTS = "d_s0 d_se d_sa_inv d_keep d_candidate d_active d_k_0".split()
OUTPUTS = "d_order d_q_pick d_rank d_q d_count d_status d_dfs_gain d_post_cov d_post_var".split()


def rec(**kw):
    kw.setdefault("nsel", 1)
    return record(CLS, **kw)


def value(r, name):
    return r.d_k[int(name[-1])] if name.startswith("d_k_") else getattr(r, name)


def test_the_mirror_is_the_record():
    assert ctypes.sizeof(CLS) == 176 and CLS.d_k.offset == MINIMUM and CLS.d_s0.offset == 56 and CLS.d_post_var.offset == 168
    assert [name for name, _ in CLS._fields_[:6]] == ["struct_size", "nblk", "se_per_profile", "s0_per_profile", "nsel", "reserved"]
    assert [name for name, _ in CLS._fields_[7:]] == [
        "d_s0", "d_se", "d_sa_inv", "d_keep", "d_candidate", "d_active", "d_order", "d_q_pick", "d_rank", "d_q", "d_count",
        "d_status", "d_dfs_gain", "d_post_cov", "d_post_var"]
    # the sibling records have not grown
    assert ctypes.sizeof(_native.MwrtOeNform) == 240 and ctypes.sizeof(_native.MwrtOeNformChar) == 168


def test_refusals_their_messages_and_their_order(record_dump):
    e = "select"
    r0 = rec()
    cases = [
        (line(e, 3, 2, 3, rec()), OK, None, rec()),
        (line(e, 0, 1, 1, rec(nblk=4)), OK, None),
        (line(e, 1, 2, 3, rec(se_per_profile=1, s0_per_profile=1, nsel=3)), OK, None),
        # the limit is on n = nblk nlev, not on m
        (line(e, 1, MAX_N, 3, rec()), OK, None),
        (line(e, 1, 32, 3, rec(nblk=4)), OK, None),
        (line(e, 1, 2, 2 ** 31 - 1, rec(nsel=2 ** 31 - 1)), OK, None),
        (line(e, 2 ** 31 - 1, 2, 3, rec()), OK, None),
        (line(e, 1, MAX_N + 1, 3, rec()), UNSUPPORTED, N_LIMIT),
        (line(e, 1, 65, 3, rec(nblk=2)), UNSUPPORTED, N_LIMIT),
        (line(e, 1, 2 ** 31 - 1, 3, rec(nblk=4)), UNSUPPORTED, N_LIMIT),
        (line(e, 2 ** 31, 2, 3, rec()), UNSUPPORTED, "nprof exceeds grid limit"),
        (line(e, 1, 2, 3, rec(struct_size=MINIMUM - 1)), INVALID, TOO_SMALL),
        (line(e, 1, 2, 3, rec(struct_size=0)), INVALID, TOO_SMALL),
        (line(e, -1, 2, 3, rec()), INVALID, SIGNS),
        (line(e, 1, 0, 3, rec()), INVALID, SIGNS),
        (line(e, 1, 2, 0, rec()), INVALID, SIGNS),
        (line(e, 1, 2, 3, rec(nblk=0)), INVALID, NBLK),
        (line(e, 1, 2, 3, rec(nblk=5)), INVALID, NBLK),
        (line(e, 1, 2, 3, rec(reserved=1)), INVALID, RESERVED),
        (line(e, 1, 2, 3, rec(nsel=0)), INVALID, NSEL),
        (line(e, 1, 2, 3, rec(nsel=-1)), INVALID, NSEL),
        (line(e, 1, 2, 3, rec(nsel=4)), INVALID, NSEL),
        (line(e, 1, 2, 3, rec(nsel=3)), OK, None),
        # two checks would fire: the earlier one is reported
        (line(e, -1, 2, 3, rec(struct_size=MINIMUM - 1)), INVALID, TOO_SMALL),
        (line(e, -1, 2, 3, rec(nblk=0)), INVALID, SIGNS),
        (line(e, 1, 2, 3, rec(nblk=5, reserved=1)), INVALID, NBLK),
        (line(e, 1, 2, 3, rec(reserved=1, nsel=0)), INVALID, RESERVED),
        (line(e, 1, 2, 3, rec(nsel=0, d_s0=None)), INVALID, NSEL),
        (line(e, 1, 2, 3, rec(d_s0=None, d_sa_inv=None)), INVALID, "null buffer"),
        (line(e, 1, 2, 3, rec(d_sa_inv=None, d_q=r0.d_se)), INVALID, DFS),
        (line(e, 1, MAX_N + 1, 3, rec(d_s0=None)), INVALID, "null buffer"),
        (line(e, 1, MAX_N + 1, 3, rec(d_q=r0.d_se)), INVALID, ALIASED),                        # the limits come last
        (line(e, 2 ** 31, MAX_N + 1, 3, rec()), UNSUPPORTED, N_LIMIT),
        # the shortest record: nsel is read, no pointer is
        (line(e, 1, 2, 3, rec(struct_size=MINIMUM)), INVALID, "null buffer"),
        (line(e, 1, 2, 3, rec(struct_size=MINIMUM, nsel=0)), INVALID, NSEL),
        # a record that ends inside the last required pointer: it reads as NULL
        (line(e, 1, 2, 3, rec(struct_size=CLS.d_status.offset + 7)), INVALID, "null buffer"),
        # one that ends behind it: the optional outputs read as NULL, and so d_dfs_gain asks for nothing
        (line(e, 1, 2, 3, rec(struct_size=CLS.d_status.offset + 8, d_sa_inv=None)), OK, None),
        (line(e, 1, 2, 3, rec(struct_size=CLS.d_dfs_gain.offset + 8, d_sa_inv=None)), INVALID, DFS),
        # d_sa_inv without d_dfs_gain is never read, and allowed
        (line(e, 1, 2, 3, rec(d_dfs_gain=None)), OK, None),
        (line(e, 1, 2, 3, rec(d_dfs_gain=None, d_sa_inv=None)), OK, None),
        (line(e, 1, 2, 3, rec(nblk=2, d_k_1=None)), INVALID, "null buffer"),
        (line(e, 1, 2, 3, rec(nblk=2, d_k_2=None, d_k_3=None)), OK, None),                     # beyond nblk: not looked at
    ]
    cases += [(line(e, 1, 2, 3, rec(**{p: None})), INVALID, "null buffer") for p in REQUIRED]
    cases += [(line(e, 1, 2, 3, rec(**{p: None})), OK, None) for p in OPTIONAL]
    cases += [(line(e, 1, 2, 3, rec(**{o: value(r0, i)})), INVALID, ALIASED) for o in OUTPUTS for i in INPUTS]
    cases += [
        (line(e, 1, 2, 3, rec(nblk=2, d_q=r0.d_k[1])), INVALID, ALIASED),
        (line(e, 1, 2, 3, rec(d_q=r0.d_k[1])), OK, None),                                      # beyond nblk
        (line(e, 1, 2, 3, rec(d_post_cov=r0.d_post_var)), OK, None),                           # outputs are not compared
    ]
    run(record_dump, cases)
