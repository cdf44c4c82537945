"""Every kernel instantiation compiled into libmwrt.so, reached by a case of its own and checked there.

Each template instantiation is its own code object (register allocation, spills, launch bounds), and the host routing
picks exactly one per stage from the frequency count (chunk width 8 / 14 / 16), the level count (workgroup class 256 /
512 / 1024, or the tau kernels' 63 levels per wave), the options (TB only, OPT, FULL, ALPHA), the frequency grid
(windowed or not) and the elevation count (k_rte_tau<NA>).

CPU part (unmarked): ``kernel_inventory`` lists the kernels of the built library with ``nm``; ``expected_kernels``
restates the routing in a few lines of Python; the union over the case table ``CASES`` must equal the inventory, in both
directions, so a new instantiation without a covering case, or a case claiming a kernel that does not exist, fails here.
The kernels in namespaces of their own (mwrt::oe, mwrt::nf, ...) are pinned by the tests of their units; the whole library,
namespace by namespace, is held against those sets and the union above in one test.
The restatement is held to the library's own planning code: ``tests/plan_dump.cpp`` links ``csrc/mwrt_plan.cpp`` as is
(a host-only unit), is built with the host compiler under ASan + UBSan and answers every seam and every case.

GPU part (each test marked ``gpu``): every case runs through its entry point and is compared with the C oracle
(TBs to 1e-6 K, optical depths and absorption to 1e-9 relative), with oracle-free checks on the tall classes against
the well-covered 256-thread ones (zero-thickness padding, chunk-width agreement).  ``tools/kernel_coverage.py`` holds a
``rocprofv3 --kernel-trace --stats`` run of this module against the inventory.  Set MWRT_MAXDEV_JSON to a path to get the
measured maximum deviation of each case family written there."""
import collections
import dataclasses
import json
import os
import re

import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
from kernel_unit import library_kernels
from plan_dump_tool import plan_dump, request as line          # noqa: F401 (plan_dump: the fixture, sanitised build)
# the kernel units with a namespace of their own: each test module names it (NAMESPACE) and pins its kernels (KERNELS)
import test_basis_kernel_resources, test_nform_char_kernel_resources, test_nform_kernel_resources    # noqa: E401
import test_obs_kernel_resources, test_oe_char_kernel_resources, test_oe_kernel_resources          # noqa: E401
import test_oe_lm_kernel_resources, test_param_kernel_resources, test_ray_kernel_resources         # noqa: E401
import test_select_kernel_resources, test_whiten_kernel_resources                                   # noqa: E401

KERNEL_UNITS = (test_basis_kernel_resources, test_nform_char_kernel_resources, test_nform_kernel_resources,
                test_obs_kernel_resources, test_oe_char_kernel_resources, test_oe_kernel_resources, test_oe_lm_kernel_resources,
                test_param_kernel_resources, test_ray_kernel_resources, test_select_kernel_resources, test_whiten_kernel_resources)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")

# ---------------------------------------------------------------------------------------------------------------------
# the routing, restated (the planning code itself: csrc/mwrt_plan.h, csrc/mwrt_plan.cpp; test_mirror_matches_the_planning_code)
# ---------------------------------------------------------------------------------------------------------------------
WAVE = 64
MAX_LEVELS = 1024
TAU_NFC = 16
WIN_CHUNKS, WIN_NFC, WIN_NODES, WIN_NODES_H = 8, 16, 16, 8
WIN_MAX_SPAN_GHZ = 6.0
NFK, WIN_CHUNKS_MAX, RTE_THREADS, MAX_MULTI, MAX_ANGLES = 8, 16, 256, 8, 64
LDS_MAX = 160 * 1024          # hipDeviceAttributeMaxSharedMemoryPerBlock on gfx950 (test_lds_budget_as_mirrored)
ERR_UNSUPPORTED = -5

TB_ONLY, OPT, FULL, ALPHA = "tb", "opt", "full", "alpha"
_FLAGS = {TB_ONLY: (False, False, False), OPT: (True, False, False), FULL: (True, True, False), ALPHA: (False, False, True)}


def roundup(n, k=WAVE):
    return -(-n // k) * k


def size_class(threads):
    """launch_by_size / launch_absorb_nfc* / launch_absorb_tau: MAXT of the instantiation a workgroup of `threads` runs"""
    return 256 if threads <= 256 else (512 if threads <= 512 else 1024)


def pick_nfc(nf):
    """pick_nfc: 14 HATPRO channels fit one chunk; other counts use 16 / 8"""
    if nf % 14 == 0 or nf <= 14:
        return 8 if nf <= 8 else 14
    return 16


def fused_lds_bytes_min(nfc, nlev, nf, nang, threads):
    """fused_lds_bytes at one segment per pass: where plan_fused's shrink loop ends, so plan_fused fails iff this does not fit"""
    nfk = NFK
    rows0, rows1 = min(nfk, nfc, nf), max(0, min(nfc, nf) - nfk)
    ldrow = nlev + 1 + ((nlev + 1) % 2 == 0)                       # plan_k2: odd row stride
    npart = 2 * nang * max(rows0, rows1)
    sort_doubles = (nfk * (threads // 16) + threads // WAVE + threads + 1) // 2
    return 8 * (2 * nfk * ldrow + npart + 16 + (threads // WAVE) * 2 * nfc + sort_doubles)


def pick_nfc_fused(nlev, nf, nang, chunk_width, lds_max):
    """pick_nfc_fused: the pinned width or pick_nfc, and 8 if the wide chunk's LDS rows cannot fit"""
    nfc = chunk_width or pick_nfc(nf)
    return nfc if fused_lds_bytes_min(nfc, nlev, nf, nang, roundup(nlev)) <= lds_max else 8


def fused_threads(nlev, nang, variant):
    """launch_fused: one lane per level in whole waves; an ALPHA workgroup with nang > 1 is padded to 256 lanes"""
    threads = roundup(nlev)
    if variant == ALPHA and threads < 256 and nang > 1:
        threads = 256
    return threads


def tau_threads(nlev):
    """tau_threads (mwrt_plan.h): 63 levels per wave plus one repeated level"""
    return -(-(nlev - 1) // (WAVE - 1)) * WAVE


def windows_eligible(frq):
    """windows_eligible: >= 128 strictly increasing frequencies, every 128-frequency window <= 6 GHz wide"""
    per = WIN_CHUNKS * WIN_NFC
    if len(frq) < per or not (np.diff(frq) > 0).all():
        return False
    for b in range(0, len(frq), per):
        e = min(len(frq), b + per) - 1
        if e == b or frq[e] - frq[b] > WIN_MAX_SPAN_GHZ:
            return False
    return True


def absorb_win_lds_bytes(threads):
    """absorb_win_lds_bytes"""
    maxt = 256 if threads <= 256 else 512
    return 8 * ((WIN_NODES + WIN_NODES_H) * threads + (3 * WIN_NFC + 2) * (1 + maxt // WAVE) + (3 * WIN_NODES_H + 2)) + 64


def windowed_ok(frq, threads, lds_max):
    """absorption_route: can the windowed kernel serve the call"""
    return windows_eligible(frq) and threads <= 512 and absorb_win_lds_bytes(threads) <= lds_max


def rte_tau_split(nang):
    """rte_tau_angles, as rte_tau_launch walks it: elevations per k_rte_tau<NA> launch -- up to 8, 10 whole, 9 as 5 + 4"""
    out, rem = [], nang
    while rem > 0:
        na = rem if rem <= 8 else (10 if rem == 10 else (5 if rem == 9 else 8))
        out.append(na)
        rem -= na
    return out


def fused_name(nfc, maxt, variant):
    return "k_tb_fused<%d, 8, %d, %s, %s, %s>" % ((nfc, maxt) + tuple("true" if f else "false" for f in _FLAGS[variant]))


def _absorb(nlev, frq, mode, lds_max):
    """mwrt_absorption_batch_device: windowed kernel (roundup(nlev) lanes) where it qualifies and mode != 1, else every line"""
    threads = roundup(nlev)
    eligible = windowed_ok(frq, threads, lds_max)
    if mode == 2 and not eligible:
        return None
    if eligible and mode != 1:
        return {"k_absorb_win<%d, false>" % size_class(threads)}
    return {"k_absorb<%d, %d, false>" % (pick_nfc(len(frq)), size_class(threads))}


def _rte(nang):
    return {"k_rte_tau<%d>" % na for na in rte_tau_split(nang)}


@dataclasses.dataclass(frozen=True)
class Call:
    """One GPU call as data.  entry: "tb" (mwrt_tb_batch[_opt]), "multi" (mwrt_tb_batch_multi), "alpha"
    (mwrt_absorption_batch_device -> mwrt_tb_from_absorption_device), "absorption" (mwrt_absorption_batch), "layer_tau"
    (mwrt_layer_tau_batch_device -> mwrt_tb_from_layer_tau_device), "jacobian" (mwrt_tb_jacobian_batch), "jacobian_device"
    (mwrt_tb_jacobian_batch_device), "selftest" (mwrt_selftest_math), "helpers" (mwrt_selftest_helpers, every selector).
    check: the GPU test that runs it."""
    check: str
    entry: str
    nlev: int
    frq: str = "hatpro"
    nang: int = 3
    options: tuple = ()            # "clouds", "rays", "ozone", "extras"
    chunk_width: int = 0
    absorption_mode: int = 0
    nmodels: int = 1
    model: str = "R24"

    def __str__(self):
        bits = [self.entry, str(self.nlev), self.frq, "a%d" % self.nang] + list(self.options)
        bits += ["w%d" % self.chunk_width] if self.chunk_width else []
        bits += ["m%d" % self.absorption_mode] if self.absorption_mode else []
        return "-".join(bits + [self.model])


def tb_variant(options):
    """tb_launch: extras -> FULL, any option -> OPT, else TB only"""
    return FULL if "extras" in options else (OPT if set(options) & {"clouds", "rays", "ozone"} else TB_ONLY)


def route(c, lds_max=LDS_MAX):
    """-> (kernel names the call launches, return code): the host routing of csrc/mwrt.hip, csrc/mwrt_plan.cpp and
    csrc/mwrt_inst.hip"""
    frq = FREQS[c.frq]
    nf = len(frq)
    if c.entry == "selftest":
        return {"k_selftest_math"}, 0
    if c.entry == "helpers":                                       # launch_selftest_helpers: one kernel per group of selectors
        return {"k_selftest_" + g for g in ("poly", "cplx", "planck", "layer", "layer4", "div_small", "block", "votes")}, 0
    if c.entry in ("jacobian", "jacobian_device"):
        return {"k_absorb_tl", "k_jac_rte"}, 0
    if c.entry == "absorption":
        ks = _absorb(c.nlev, frq, c.absorption_mode, lds_max)
        return (set(), ERR_UNSUPPORTED) if ks is None else (ks, 0)
    if c.entry == "layer_tau":                                     # layer_tau_launch
        threads = tau_threads(c.nlev)
        eligible = threads <= 1024 and windowed_ok(frq, threads, lds_max)
        if threads > 1024 or (c.absorption_mode == 2 and not eligible):
            return set(), ERR_UNSUPPORTED
        if eligible and c.absorption_mode != 1:
            k1 = "k_absorb_win<%d, true>" % size_class(threads)
        else:
            k1 = "k_absorb<%d, %d, true>" % (TAU_NFC, size_class(threads))
        return {k1} | _rte(c.nang), 0
    if c.entry == "alpha":
        nfc = pick_nfc_fused(c.nlev, nf, c.nang, c.chunk_width, lds_max)
        return _absorb(c.nlev, frq, 0, lds_max) | {fused_name(nfc, size_class(fused_threads(c.nlev, c.nang, ALPHA)), ALPHA)}, 0
    # "tb" / "multi": tb_launch
    variant = tb_variant(c.options)
    ks = {"k_ray_paths"} if "rays" in c.options else set()
    if variant == TB_ONLY and c.nmodels == 1 and c.absorption_mode != 1 and windowed_ok(frq, tau_threads(c.nlev), lds_max):
        return ks | {"k_absorb_win<%d, true>" % size_class(tau_threads(c.nlev))} | _rte(c.nang), 0
    nfc = pick_nfc_fused(c.nlev, nf, c.nang, c.chunk_width, lds_max)
    return ks | {fused_name(nfc, size_class(fused_threads(c.nlev, c.nang, variant)), variant)}, 0


def expected_kernels(c, lds_max=LDS_MAX):
    return route(c, lds_max)[0]


_KERNEL_RE = re.compile(r"mwrt::(?:\(anonymous namespace\)::)?(k_\w+(?:<[^>()]*>)?)\(")


def normalise_kernel_name(symbol):
    """'void mwrt::k_absorb<16, 1024, true>(mwrt::AbsorbArgs)' -> 'k_absorb<16, 1024, true>'; None for other symbols"""
    if "__device_stub__" in symbol:
        return None
    m = _KERNEL_RE.search(symbol)
    return m.group(1) if m else None


def kernel_inventory(lib_path):
    """The kernels compiled into `lib_path` directly in mwrt: the host handles of mwrt::k_* (anonymous-namespace ones
    included).  The units' own namespaces are beside them in library_kernels(lib_path)."""
    return library_kernels(lib_path)[""]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
FREQS = {
    "f8": np.array([22.24, 23.84, 31.4, 51.26, 53.86, 56.66, 58.0, 89.0]),                # one 8-wide chunk
    "hatpro": pr.HATPRO_FRQS,                                                             # one 14-wide chunk
    "f33": np.sort(np.concatenate([pr.HATPRO_FRQS, [10.7, 18.7, 36.5, 60.3061, 72.5, 89.0, 90.0, 110.0, 118.7503, 122.0,
                                                    150.0, 166.0, 175.31, 180.31, 183.31, 186.31, 190.31, 229.0, 325.15]])),
    "fine": pr.fine_grid_frequencies(1000)[300:812],      # 512 frequencies, 128-frequency windows 5.1 GHz wide
}
FAMILIES = ["R98", "R17", "R20", "R20SD", "R24"]


def angles(nang, low=False):
    if nang == 1:
        return np.array([90.0])
    return np.linspace(90.0, 4.2 if low else 5.4, nang)


def _build_cases():
    cases = []

    def add(check, entry, nlev, **kw):
        kw.setdefault("model", FAMILIES[len(cases) % len(FAMILIES)])
        cases.append(Call(check, entry, nlev, **kw))

    # every fused variant at every width (from the frequency count) and every size class, at the wave / class seams;
    # OPT carries clouds, rays at low elevations and, at width 16, ozone; FULL carries clouds and every extras column
    for opts, nang in (((), 3), (("clouds", "rays"), 4), (("clouds", "extras"), 3)):
        for frq in ("f8", "hatpro", "f33"):
            for nlev in (2, 63, 64, 65, 256, 257, 512, 513, 1024):
                o = opts + (("ozone",) if "rays" in opts and frq == "f33" else ())
                add("fused", "tb", nlev, frq=frq, nang=nang, options=o)
    # RTE from absorption: 3 / 2 / 1 / 0 dead waves under the 256-lane pad (nang > 1), no pad (nang == 1), tall classes
    for k, nlev in enumerate((2, 64, 65, 128, 129, 192, 193, 257, 512, 600, 1024)):
        for j, nang in enumerate((1, 4)):
            add("alpha", "alpha", nlev, frq=("f8", "hatpro", "f33")[(2 * k + j) % 3], nang=nang)
    # fine grid, automatic: windowed tau kernel at the tau seams, the fused kernel from 506 levels on
    for nlev in (253, 254, 505, 506):
        add("fine_tb", "tb", nlev, frq="fine", nang=7)
    # every k_rte_tau<NA>
    for nang in (1, 2, 3, 4, 6, 7, 8, 9, 10, 14):
        add("rte", "tb", 180, frq="fine", nang=nang)
    # the public layer-tau pair, every-line form at the tau seams; refused above 1009 levels
    for nlev in (253, 254, 505, 1009, 1010):
        add("layer_tau", "layer_tau", nlev, frq="fine", nang=2, absorption_mode=1)
    # absorption on the fine grid: windowed at its class seam (modes 0 and 2), every line beyond it, refused in mode 2
    for nlev in (256, 257, 512):
        for mode in (0, 2):
            add("absorption", "absorption", nlev, frq="fine", absorption_mode=mode)
    add("absorption", "absorption", 513, frq="fine", absorption_mode=2)
    add("absorption", "absorption", 1024, frq="fine")
    # all 8 model slots over three 16-wide chunks
    for nlev in (180, 600):
        add("multi", "multi", nlev, frq="f33", nmodels=8)
    # zero-thickness padding of a 180-level profile, and chunk-width agreement, on the tall classes
    for variant, entry, opts in ((TB_ONLY, "tb", ()), (FULL, "tb", ("clouds", "extras")), (ALPHA, "alpha", ())):
        for nlev in (600, 1024):
            add("padding", entry, nlev, options=opts, model="R24")
    for variant, entry, opts in ((TB_ONLY, "tb", ()), (OPT, "tb", ("clouds", "rays")), (FULL, "tb", ("clouds", "extras")),
                                 (ALPHA, "alpha", ())):
        for w in (8, 14, 16):
            add("widths", entry, 1024, frq="f33", options=opts, chunk_width=w, model="R17")
    # one small call each to the remaining kernels, at 1024 levels
    add("misc", "selftest", 2, model="R24")
    add("helpers", "helpers", 2, model="R24")
    add("misc", "jacobian", 1024, nang=2, model="R24")
    add("misc", "jacobian_device", 1024, nang=2, model="R24")
    add("misc", "tb", 1024, options=("rays",), nang=4, model="R24")
    return cases


CASES = _build_cases()


def cases_of(check):
    return [c for c in CASES if c.check == check]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the mirror and the inventory
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_compiled_kernel(native_lib):
    inventory = kernel_inventory(native_lib._name)
    claimed = set().union(*(expected_kernels(c) for c in CASES))
    assert inventory, "nm found no mwrt::k_* kernel in the library"
    assert not inventory - claimed, "compiled kernels no case reaches: %s" % sorted(inventory - claimed)
    assert not claimed - inventory, "cases claim kernels that are not compiled: %s" % sorted(claimed - inventory)


def test_the_library_holds_the_units_kernels_and_no_other(native_lib):
    """Every kernel of libmwrt.so, namespace by namespace, against what the tests of the units pin: a kernel in a namespace
    no unit lists, or in a unit's namespace under another unit's name, fails here."""
    table = {unit.NAMESPACE: unit.KERNELS for unit in KERNEL_UNITS}
    assert len(table) == len(KERNEL_UNITS)
    table[""] = set().union(*(expected_kernels(c) for c in CASES))
    found = library_kernels(native_lib._name)
    assert found == table, {ns: sorted(found.get(ns, set()) ^ table.get(ns, set())) for ns in set(found) | set(table)
                            if found.get(ns) != table.get(ns)}


# what test_routing_mirror_at_its_seams pins, as inputs: the planning code is asked the same questions
SEAM_NLEV = (2, 64, 65, 253, 254, 505, 506, 1009, 1010)
SEAM_NANG = (1, 6, 8, 9, 10, 14, 64)
SEAM_NF = (1, 8, 9, 14, 15, 16, 28, 33, 42, 512)


def seam_frequency_lists():
    f = FREQS["fine"]
    return [f, f[:127], f[::-1], np.linspace(20.0, 26.1, 128), np.linspace(20.0, 26.0, 128), f[:129]]


def test_mirror_matches_the_planning_code(plan_dump, tmp_path):
    """The Python restatement above against csrc/mwrt_plan.cpp itself, at every seam of test_routing_mirror_at_its_seams and
    for every Call of CASES; the same sanitised run takes the frequency lists through chunk_masks and build_windows"""
    want, asked = [], []

    def ask(request, expect):
        asked.append(request)
        want.append(expect)

    ask("constants", dict(WAVE=WAVE, NFK=NFK, TAU_NFC=TAU_NFC, WIN_CHUNKS=WIN_CHUNKS, WIN_CHUNKS_MAX=WIN_CHUNKS_MAX, WIN_NFC=WIN_NFC,
                          WIN_NODES=WIN_NODES, WIN_NODES_H=WIN_NODES_H, WIN_MAX_SPAN_GHZ=WIN_MAX_SPAN_GHZ, RTE_THREADS=RTE_THREADS,
                          MAX_MULTI=MAX_MULTI, MAX_LEVELS=MAX_LEVELS, MAX_ANGLES=MAX_ANGLES, ERR_UNSUPPORTED=ERR_UNSUPPORTED))

    def fused(nlev, nf, nang, width, lds_max, threads):
        nfc = pick_nfc_fused(nlev, nf, nang, width, lds_max)
        ask(line("fused", nlev, nf, nang, width, lds_max, threads),
            dict(pick_nfc=pick_nfc(nf), nfc=nfc, fits=fused_lds_bytes_min(nfc, nlev, nf, nang, threads) <= lds_max,
                 lds_min_wide=fused_lds_bytes_min(width or pick_nfc(nf), nlev, nf, nang, threads)))

    def levels(nlev):
        ask(line("tau", nlev), dict(tau_threads=tau_threads(nlev), lanes_for=roundup(nlev)))

    for nlev in SEAM_NLEV:
        levels(nlev)
    for threads in range(WAVE, MAX_LEVELS + 2 * WAVE, WAVE):
        ask(line("winlds", threads), dict(absorb_win_lds_bytes=absorb_win_lds_bytes(threads)))
    for nang in SEAM_NANG + tuple(range(1, MAX_ANGLES + 1)):
        ask(line("split", nang), dict(split=rte_tau_split(nang)))
    for nf in SEAM_NF:
        fused(180, nf, 3, 0, LDS_MAX, roundup(180))
    for lds_max in (64 * 1024, LDS_MAX):
        fused(1024, 33, 64, 0, lds_max, 1024)
    for f in seam_frequency_lists():
        ask(line("eligible", *f), dict(eligible=windows_eligible(f)))
    for c in CASES:
        frq = FREQS[c.frq]
        variant = ALPHA if c.entry == "alpha" else tb_variant(c.options)
        levels(c.nlev)
        ask(line("split", c.nang), dict(split=rte_tau_split(c.nang)))
        ask(line("eligible", *frq), dict(eligible=windows_eligible(frq)))
        for lds_max in (64 * 1024, LDS_MAX):
            fused(c.nlev, len(frq), c.nang, c.chunk_width, lds_max, fused_threads(c.nlev, c.nang, variant))
    # chunk_masks / build_windows / pack_windows under the sanitisers: every table family x four frequency lists
    fine = FREQS["fine"]
    for family in FAMILIES:
        path = tmp_path / (family + ".desc")
        path.write_bytes(bytes(sp.get_model(family).to_c()))
        ask(line("tables", path), {})
        for f in (FREQS["hatpro"], fine, fine[:129], fine[:16]):
            nchunks = [-(-len(f) // w) for w in (8, 14, 16)]
            ask(line("blobs", *f), dict(nchunks=nchunks, window_chunks=nchunks[2]))
    got = plan_dump(asked)
    assert got[0]["sizeof_desc"] == len(bytes(sp.get_model("R24").to_c()))
    for request, g, w in zip(asked, got, want):
        assert {k: g[k] for k in w} == w, (request[:80], g, w)
        if request.startswith("blobs"):
            off = g["layout"]
            assert g["nwin"] >= 1 and g["blob_bytes"] == off[3] and all(o % 256 == 0 for o in off) and 0 < off[0] < off[1] < off[2] < off[3]
            assert g["flo"] in [float(x) for x in request.split()[1:]]
    assert "#define MWRT_MAX_LEVELS %d" % MAX_LEVELS in open(os.path.join(ROOT, "include", "mwrt.h")).read()


def test_routing_mirror_at_its_seams():
    assert [tau_threads(n) for n in SEAM_NLEV] == [64, 64, 128, 256, 320, 512, 576, 1024, 1088]
    assert [size_class(tau_threads(n)) for n in (253, 254, 505, 506, 1009)] == [256, 512, 512, 1024, 1024]
    fine = lambda nlev, **kw: Call("x", "layer_tau", nlev, frq="fine", nang=2, **kw)
    assert route(fine(1009, absorption_mode=1)) == ({"k_absorb<16, 1024, true>", "k_rte_tau<2>"}, 0)
    assert route(fine(1010, absorption_mode=1)) == (set(), ERR_UNSUPPORTED)
    assert route(fine(505)) == ({"k_absorb_win<512, true>", "k_rte_tau<2>"}, 0)
    assert route(fine(506)) == ({"k_absorb<16, 1024, true>", "k_rte_tau<2>"}, 0)      # too tall for the windows
    assert route(fine(506, absorption_mode=2))[1] == ERR_UNSUPPORTED
    assert [rte_tau_split(n) for n in SEAM_NANG] == [[1], [6], [8], [5, 4], [10], [8, 6], [8] * 8]
    assert [pick_nfc(n) for n in SEAM_NF] == [8, 8, 14, 14, 16, 16, 14, 16, 14, 16]
    assert [fused_threads(n, 2, ALPHA) for n in (2, 64, 65, 128, 129, 192, 193, 600)] == [256] * 7 + [640]
    assert [fused_threads(n, 1, ALPHA) for n in (2, 64, 65, 193)] == [64, 64, 128, 256]
    assert fused_threads(64, 2, TB_ONLY) == 64
    f = FREQS["fine"]
    assert windows_eligible(f) and not windows_eligible(f[:127]) and not windows_eligible(f[::-1])
    assert not windows_eligible(np.linspace(20.0, 26.1, 128)) and windows_eligible(np.linspace(20.0, 26.0, 128))
    assert not windows_eligible(f[:129])                          # a one-frequency last window
    tb = lambda nlev, **kw: Call("x", "tb", nlev, frq="fine", nang=7, **kw)
    assert route(tb(505)) == ({"k_absorb_win<512, true>", "k_rte_tau<7>"}, 0)
    assert route(tb(506)) == ({"k_tb_fused<16, 8, 512, false, false, false>"}, 0)      # silent fall-back to the fused kernel
    assert route(tb(253, absorption_mode=1)) == ({"k_tb_fused<16, 8, 256, false, false, false>"}, 0)
    assert route(tb(253, options=("extras",))) == ({"k_tb_fused<16, 8, 256, true, true, false>"}, 0)
    assert route(Call("x", "absorption", 512, frq="fine")) == ({"k_absorb_win<512, false>"}, 0)
    assert route(Call("x", "absorption", 513, frq="fine")) == ({"k_absorb<16, 1024, false>"}, 0)
    # the widest LDS plan -- 1024 levels x 64 elevations at width 16 -- fits 160 KB at one segment per pass
    assert 140_000 < fused_lds_bytes_min(16, 1024, 33, 64, 1024) <= LDS_MAX
    assert pick_nfc_fused(1024, 33, 64, 0, 64 * 1024) == 8 and pick_nfc_fused(1024, 33, 64, 0, LDS_MAX) == 16


# ---------------------------------------------------------------------------------------------------------------------
# GPU: each case against the oracle
# ---------------------------------------------------------------------------------------------------------------------
TOL_K = 1e-6                  # TB vs the oracle (tests/test_gpu_parity.py)
TOL_REL = 1e-9                # optical depths, absorption
MAXDEV = collections.defaultdict(float)


def record(family, value):
    MAXDEV[family] = max(MAXDEV[family], float(value))


@pytest.fixture(scope="module", autouse=True)
def _report_maxdev():
    yield
    if MAXDEV:
        print("\nmaximum deviation per case family:\n" + "\n".join("  %-28s %.3e" % kv for kv in sorted(MAXDEV.items())))
        path = os.environ.get("MWRT_MAXDEV_JSON")
        if path:
            with open(path, "w") as f:
                json.dump(dict(sorted(MAXDEV.items())), f, indent=1)


def relerr(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0))


def profiles(nlev, seed, nprof=2):
    """[nprof][nlev] synthetic profiles; below 20 levels, levels picked from a 20-level one (ground and top kept)"""
    n = max(nlev, 20)
    P = pr.synthetic_profiles(nprof, seed, nlev=n)
    if nlev < n:
        idx = np.round(np.linspace(0, n - 1, nlev)).astype(int)
        P = {k: np.ascontiguousarray(v[:, idx]) for k, v in P.items()}
    return P


def clouds(nprof, nlev, seed):
    """liquid in the lower third, ice above mid-column, every profile"""
    rng = np.random.default_rng(seed)
    lwc, iwc = np.zeros((nprof, nlev)), np.zeros((nprof, nlev))
    for i in range(nprof):
        b = int(rng.integers(0, max(1, nlev // 3)))
        w = max(1, nlev // 10)
        lwc[i, b:b + w] = rng.uniform(0.05, 0.5, len(lwc[i, b:b + w]))
        bi = nlev // 2
        iwc[i, bi:bi + max(1, nlev // 12)] = rng.uniform(0.005, 0.05, len(iwc[i, bi:bi + max(1, nlev // 12)]))
    return lwc, iwc


_O3 = {}


def ozone_model(base):
    """`base` with a synthetic extra-species line table, built the way tools/fuzz_parity.py builds one (a line on a channel)"""
    if base not in _O3:
        rng = np.random.default_rng(7)
        nx = 6
        fl = np.sort(rng.uniform(15.0, 200.0, nx))
        fl[0] = 31.4 + 0.01
        _O3[base] = sp.get_model(base).with_extra_lines(
            dict(fl=fl, s1=10 ** rng.uniform(-13.5, -11.5, nx), b=rng.uniform(0.1, 3.0, nx), w=rng.uniform(1.8e-3, 3.2e-3, nx),
                 x=rng.uniform(0.5, 0.9, nx)), name=f"{base}_o3_instantiations")
    return _O3[base]


def o3_density(P):
    return sp.number_density_from_ppmv(np.where(P["z"] > 15.0, 5.0, 0.1), P["p"], P["t"])


class chunk_width:
    """set_chunk_width for one call, the automatic choice restored whatever happens"""

    def __init__(self, ctx, width):
        self.ctx, self.width = ctx, width

    def __enter__(self):
        self.ctx.set_chunk_width(self.width)

    def __exit__(self, *exc):
        self.ctx.set_chunk_width(0)


class absorption_mode(chunk_width):
    def __enter__(self):
        self.ctx.set_absorption_mode(self.width)

    def __exit__(self, *exc):
        self.ctx.set_absorption_mode(0)


def tables_of(c):
    return ozone_model(c.model) if "ozone" in c.options else sp.get_model(c.model)


def run_tb(ctx, c, P, ang, opt_inputs=None):
    """the case's tb call -> (tb, valid, extras or None)"""
    kw = dict(opt_inputs or {})
    with chunk_width(ctx, c.chunk_width), absorption_mode(ctx, c.absorption_mode):
        r = ctx.tb_batch(tables_of(c), P["z"], P["p"], P["t"], P["rh"], FREQS[c.frq], ang, extras="extras" in c.options, **kw)
    return r if len(r) == 3 else (r[0], r[1], None)


def opt_inputs_of(c, P, seed):
    kw = {}
    if "clouds" in c.options:
        kw["denliq"], kw["denice"] = clouds(P["z"].shape[0], P["z"].shape[1], seed)
    if "rays" in c.options:
        kw["ray_tracing"] = True
    if "ozone" in c.options:
        kw["o3n"] = o3_density(P)
    return kw


def run_alpha(ctx, c, P, ang):
    """absorption_batch_device -> tb_from_absorption_device on torch buffers -> (tb, valid, awet, adry)"""
    import torch
    dev = torch.device("cuda:0")
    nprof, nlev = P["z"].shape
    frq = FREQS[c.frq]
    d = {k: torch.from_numpy(np.ascontiguousarray(P[k])).to(dev) for k in ("z", "p", "t", "rh")}
    aw = torch.full((nprof, len(frq), nlev), -7.0, dtype=torch.float64, device=dev)
    ad = torch.full_like(aw, -7.0)
    out = torch.full((nprof, len(ang), len(frq)), -7.0, dtype=torch.float64, device=dev)
    val = torch.full((nprof,), 9, dtype=torch.uint8, device=dev)
    m = tables_of(c)
    st = torch.cuda.current_stream().cuda_stream          # ordered with the fills above
    with chunk_width(ctx, c.chunk_width):
        ctx.absorption_batch_device(m, nprof, nlev, d["p"].data_ptr(), d["t"].data_ptr(), d["rh"].data_ptr(), frq,
                                    aw.data_ptr(), ad.data_ptr(), stream=st)
        ctx.tb_from_absorption_device(m, nprof, nlev, d["z"].data_ptr(), d["t"].data_ptr(), frq, ang, aw.data_ptr(),
                                      ad.data_ptr(), out.data_ptr(), val.data_ptr(), stream=st)
    return out.cpu().numpy(), val.cpu().numpy(), aw.cpu().numpy(), ad.cpu().numpy()


def oracle_opt(c, P, i, frq, ang, kw):
    """C oracle for profile i with the case's options -> dict of [nang][nf] columns, or the valid flag it implies"""
    from oracle import c_oracle as co
    t = tables_of(c)
    row = lambda k: None if kw.get(k) is None else kw[k][i]
    try:
        r = co.tb_profile_opt(t, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], frq, ang, row("denliq"), row("denice"),
                              bool(kw.get("ray_tracing")), row("o3n"))
    except ValueError as err:
        return 3 if "RayTrac" in str(err) else 2
    return {k: v.reshape(len(ang), len(frq)) for k, v in r.items()}


def logmean_layers(x, zeroflg):
    """exponential_integration's layer values [nlev] (0 for the ground level), branch for branch, with the log-mean
    taken as d / log1p(d / x0): the oracle's d / log(x1 / x0) loses ~eps / |d / x0| -- 1.3e-9 relative on a tall
    profile's dry term, where adjacent levels differ by 1e-8"""
    x1, x0 = x[1:], x[:-1]
    d = x1 - x0
    with np.errstate(divide="ignore", invalid="ignore"):
        lm = d / np.log1p(d / x0)
    lm = np.where((x0 == 0.0) | (x1 == 0.0), 0.5 * (x1 + x0) if zeroflg else 0.0, lm)
    return np.append(0.0, np.where(np.abs(d) < 1e-9, x1, lm))


def zenith_taulay(m, P, i, frq, denliq=None, denice=None):
    """zenith layer optical depths [nf][nlev] of profile i from lbl_oracle's level absorption (its `taulay`, summed the
    same way, with the accurate layer values of logmean_layers)"""
    from oracle import lbl_oracle as lo
    z, p, t, rh = (P[k][i] for k in ("z", "p", "t", "rh"))
    e, _ = lo.vapor(t, rh)
    dz = np.append(0.0, np.diff(z - z[0]))
    out = np.zeros((len(frq), len(z)))
    for j, f in enumerate(frq):
        aw, ad = lo.clearsky_absorption(m, p, t, e, f)
        lay = [logmean_layers(aw, True), logmean_layers(ad, True)]
        if denliq is not None:
            al, ai = lo.cloudy_absorption(m, t, denliq[i], denice[i], f)
            lay += [logmean_layers(ai, False), logmean_layers(al, False)]
        out[j] = sum(v * dz for v in lay)
    return out


def check_tb_rows(family, tb, valid, i, ref):
    """tb[i] against an oracle result (dict) or the flag it implies (int); NaN only where the oracle has NaN"""
    if isinstance(ref, int):
        assert valid[i] == ref and np.isnan(tb[i]).all(), (family, i, int(valid[i]), ref)
        return
    assert valid[i] == 1, (family, i, int(valid[i]))
    want = ref["tbtotal"]
    assert np.array_equal(np.isnan(tb[i]), np.isnan(want)), (family, i)
    dev = float(np.nanmax(np.abs(tb[i] - want), initial=0.0))
    record(family + " TB", dev)
    assert dev <= TOL_K, (family, i, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("fused"), ids=str)
def test_fused_variant_matches_oracle(gpu_ctx, case):
    """TB only / OPT (clouds, rays at 4.2 degrees, ozone at width 16) / FULL (every extras column) at every width and
    size class, against the C oracle; FULL's zenith layer optical depths against lbl_oracle's on a frequency subset"""
    c = case
    P = profiles(c.nlev, 40 + c.nlev)
    frq, ang = FREQS[c.frq], angles(c.nang, low="rays" in c.options)
    kw = opt_inputs_of(c, P, c.nlev)
    tb, valid, ex = run_tb(gpu_ctx, c, P, ang, kw)
    variant = tb_variant(c.options)
    for i in range(2):
        ref = oracle_opt(c, P, i, frq, ang, kw)
        check_tb_rows(variant, tb, valid, i, ref)
        if ex is None or isinstance(ref, int):
            continue
        for k in ("tbatm", "tmr"):
            dev = float(np.abs(ex[k][i] - ref[k]).max())
            record(f"{variant} {k}", dev)
            assert dev <= TOL_K, (k, i, dev)
        for k in ("tauwet", "taudry", "tauliq", "tauice"):
            assert np.allclose(ex[k][i], ref[k], rtol=TOL_REL, atol=1e-14), (k, i)
            record(f"{variant} {k} (rel)", relerr(ex[k][i][ref[k] > 1e-12], ref[k][ref[k] > 1e-12]))
        sub = np.arange(0, len(frq), 3)
        zen = zenith_taulay(tables_of(c), P, i, frq[sub], kw["denliq"], kw["denice"])
        assert np.allclose(ex["taulay"][i][sub], zen, rtol=TOL_REL, atol=1e-15), i
        record(f"{variant} taulay (rel)", relerr(ex["taulay"][i][sub][zen > 1e-12], zen[zen > 1e-12]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("alpha"), ids=str)
def test_rte_from_absorption(gpu_ctx, case):
    """ALPHA fed by absorption_batch_device: the absorption meets the oracle, the TBs meet the fused kernel to 1e-9 K
    and the oracle to 1e-6 K -- with 3, 2, 1 and 0 lane-less waves under the 256-lane pad, unpadded at nang == 1"""
    from oracle import c_oracle as co
    c = case
    P = profiles(c.nlev, 60 + c.nlev)
    frq, ang = FREQS[c.frq], angles(c.nang)
    tb, valid, aw, ad = run_alpha(gpu_ctx, c, P, ang)
    fused, fv = gpu_ctx.tb_batch(c.model, P["z"], P["p"], P["t"], P["rh"], frq, ang)
    assert (valid == 1).all() and (fv == 1).all()
    dev = float(np.abs(tb - fused).max())
    record("ALPHA vs fused", dev)
    assert dev <= 1e-9, dev
    m = sp.get_model(c.model)
    for i in range(2):
        ow, od = co.absorption_profile(m, P["p"][i], P["t"][i], P["rh"][i], frq)
        assert np.allclose(aw[i], ow, rtol=TOL_REL, atol=1e-300) and np.allclose(ad[i], od, rtol=TOL_REL, atol=1e-300), i
        record("k_absorb vs oracle (rel)", max(relerr(aw[i], ow), relerr(ad[i], od)))
        ref = co.tb_profile(m, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], frq, ang)["tbtotal"].reshape(len(ang), len(frq))
        dev = float(np.abs(tb[i] - ref).max())
        record("ALPHA TB", dev)
        assert dev <= TOL_K, (i, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("fine_tb") + cases_of("rte"), ids=str)
def test_fine_grid_tb_path(gpu_ctx, case):
    """The automatic fine-grid path (windowed tau kernel -> k_rte_tau<NA>) meets the oracle and the every-line fused call
    (absorption_mode 1) to 1e-8 K; where it falls back to the fused kernel (506 levels) the two calls are identical"""
    from oracle import c_oracle as co
    c = case
    P = profiles(c.nlev, 80 + c.nlev + c.nang)
    frq, ang = FREQS[c.frq], angles(c.nang)
    tb, valid, _ = run_tb(gpu_ctx, c, P, ang)
    direct, dv, _ = run_tb(gpu_ctx, dataclasses.replace(c, absorption_mode=1), P, ang)
    assert (valid == 1).all() and (dv == 1).all() and np.isfinite(tb).all()
    if any(k.startswith("k_tb_fused") for k in expected_kernels(c)):
        assert np.array_equal(tb, direct)
    else:
        dev = float(np.abs(tb - direct).max())
        record("fine tau path vs fused", dev)
        assert dev <= 1e-8, dev
    sub = np.arange(0, len(frq), 32)
    m = sp.get_model(c.model)
    for i in range(2):
        ref = co.tb_profile(m, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], frq[sub], ang)["tbtotal"].reshape(len(ang), len(sub))
        dev = float(np.abs(tb[i][:, sub] - ref).max())
        record("fine tau path TB", dev)
        assert dev <= TOL_K, (i, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("layer_tau"), ids=str)
def test_layer_tau_pair_at_its_seams(gpu_ctx, case):
    """mwrt_layer_tau_batch_device (every-line k_absorb<16, *, true>) -> mwrt_tb_from_layer_tau_device at 253 / 254 / 505 /
    1009 levels: zenith layer optical depths to 1e-9 relative of lbl_oracle's, TBs to the oracle and the fused kernel;
    1010 levels are refused with MWRT_ERR_UNSUPPORTED while the fused kernel serves them"""
    import torch
    from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError
    from oracle import c_oracle as co
    c = case
    P = profiles(c.nlev, 100 + c.nlev)
    frq, ang = FREQS[c.frq], angles(c.nang, low=True)
    nprof, nlev, nf = 2, c.nlev, len(frq)
    dev = torch.device("cuda:0")
    pitch = gpu_ctx.layer_tau_pitch(nf)
    d = {k: torch.from_numpy(P[k]).to(dev) for k in ("z", "p", "t", "rh")}
    tau = torch.full((nprof, nlev, pitch), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((nprof, len(ang), nf), -7.0, dtype=torch.float64, device=dev)
    val = torch.full((nprof,), 9, dtype=torch.uint8, device=dev)
    m = sp.get_model(c.model)
    st = torch.cuda.current_stream().cuda_stream          # ordered with the fills above and the copies below
    with absorption_mode(gpu_ctx, c.absorption_mode):
        if route(c)[1] == ERR_UNSUPPORTED:
            with pytest.raises(MwrtError) as ei:
                gpu_ctx.layer_tau_batch_device(m, nprof, nlev, d["z"].data_ptr(), d["p"].data_ptr(), d["t"].data_ptr(),
                                               d["rh"].data_ptr(), frq, tau.data_ptr(), pitch, val.data_ptr(), stream=st)
            assert ei.value.code == ERR_UNSUPPORTED
            assert (val.cpu().numpy() == 9).all() and (tau.cpu().numpy() == -7.0).all()       # nothing was launched
        else:
            gpu_ctx.layer_tau_batch_device(m, nprof, nlev, d["z"].data_ptr(), d["p"].data_ptr(), d["t"].data_ptr(),
                                           d["rh"].data_ptr(), frq, tau.data_ptr(), pitch, val.data_ptr(), stream=st)
            gpu_ctx.tb_from_layer_tau_device(m, nprof, nlev, tau.data_ptr(), pitch, d["t"].data_ptr(), frq, ang,
                                             val.data_ptr(), out.data_ptr(), stream=st)
        fused, fv = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ang)
    assert (fv == 1).all()
    if route(c)[1] == ERR_UNSUPPORTED:
        return
    tau, tb, v = tau.cpu().numpy()[:, :, :nf], out.cpu().numpy(), val.cpu().numpy()
    assert (v == 1).all() and (tau[:, 0, :] == 0.0).all()
    d8 = float(np.abs(tb - fused).max())
    record("layer tau pair vs fused", d8)
    assert d8 <= 1e-8, d8
    sub = np.arange(0, nf, 64)
    for i in range(2):
        zen = zenith_taulay(m, P, i, frq[sub])
        assert np.allclose(tau[i][:, sub].T, zen, rtol=TOL_REL, atol=1e-300), i
        record("layer tau (rel)", relerr(tau[i][:, sub].T[zen > 1e-12], zen[zen > 1e-12]))
        ref = co.tb_profile(m, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], frq[sub], ang)["tbtotal"]
        dev = float(np.abs(tb[i][:, sub] - ref.reshape(len(ang), len(sub))).max())
        record("layer tau pair TB", dev)
        assert dev <= TOL_K, (i, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("absorption"), ids=str)
def test_fine_grid_absorption(gpu_ctx, case):
    """mwrt_absorption_batch on the fine grid: k_absorb_win<256 | 512, false> (modes 0 and 2) and the every-line kernel beyond
    512 levels against the oracle and the every-line kernel; mode 2 refuses what the windows cannot serve"""
    from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError
    from oracle import c_oracle as co
    c = case
    P = profiles(c.nlev, 120 + c.nlev)
    frq = FREQS[c.frq]
    m = sp.get_model(c.model)
    with absorption_mode(gpu_ctx, c.absorption_mode):
        if route(c)[1] == ERR_UNSUPPORTED:
            with pytest.raises(MwrtError) as ei:
                gpu_ctx.absorption_batch(m, P["p"], P["t"], P["rh"], frq)
            assert ei.value.code == ERR_UNSUPPORTED
            return
        aw, ad = gpu_ctx.absorption_batch(m, P["p"], P["t"], P["rh"], frq)
    with absorption_mode(gpu_ctx, 1):
        dw, dd = gpu_ctx.absorption_batch(m, P["p"], P["t"], P["rh"], frq)
    assert np.allclose(aw, dw, rtol=2e-10, atol=1e-300) and np.allclose(ad, dd, rtol=2e-10, atol=1e-300)
    record("windowed vs every-line absorption (rel)", max(relerr(aw, dw), relerr(ad, dd)))
    sub = np.arange(0, len(frq), 16)
    for i in range(2):
        ow, od = co.absorption_profile(m, P["p"][i], P["t"][i], P["rh"][i], frq[sub])
        assert np.allclose(aw[i][sub], ow, rtol=TOL_REL, atol=1e-300) and np.allclose(ad[i][sub], od, rtol=TOL_REL, atol=1e-300)
        record("fine absorption vs oracle (rel)", max(relerr(aw[i][sub], ow), relerr(ad[i][sub], od)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("multi"), ids=str)
def test_eight_models_over_three_chunks(gpu_ctx, case):
    """All 8 model slots (the five table families, two fuzzed tables, one negative continuum) over nf = 33 (16 + 16 + 1):
    bit for bit the single-model calls; the negative-continuum model's rows are valid 2 and NaN in every chunk, a NaN
    profile is valid 0 in every model, the other rows meet the oracle"""
    from oracle import c_oracle as co
    from oracle.fuzz_tables import fuzzed_tables
    c = case
    neg = dataclasses.replace(sp.get_model("R98"), name="R98_negcont_instantiations", h2o_cf=-1e-6)
    models = [sp.get_model(n) for n in FAMILIES] + [fuzzed_tables(s)[0] for s in (0, 1)] + [neg]
    assert len(models) == c.nmodels == 8
    P = profiles(c.nlev, 140 + c.nlev, nprof=4)
    P["t"][2, c.nlev // 2] = np.nan
    frq, ang = FREQS[c.frq], angles(c.nang, low=True)
    tbm, vm = gpu_ctx.tb_batch_multi(models, P["z"], P["p"], P["t"], P["rh"], frq, ang)
    assert tbm.shape == (8, 4, len(ang), len(frq))
    for k, m in enumerate(models):
        tb, v = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ang)
        assert np.array_equal(v, vm[k]) and np.array_equal(tb, tbm[k], equal_nan=True), m.name
        assert vm[k][2] == 0 and np.isnan(tbm[k][2]).all(), m.name
        if m is neg:
            assert (vm[k][[0, 1, 3]] == 2).all() and np.isnan(tbm[k]).all()
            continue
        assert (vm[k][[0, 1, 3]] == 1).all() and np.isfinite(tbm[k][[0, 1, 3]]).all(), m.name
        ref = co.tb_profile(m, P["z"][k % 2], P["p"][k % 2], P["t"][k % 2], P["rh"][k % 2], frq, ang)["tbtotal"]
        dev = float(np.abs(tbm[k][k % 2].ravel() - ref).max())
        record("multi-model TB", dev)
        assert dev <= TOL_K, (m.name, dev)


def padded_index(nlev, seed):
    """indices into a 180-level profile: every level once, the rest repeats (zero-thickness layers), ground -> top"""
    rng = np.random.default_rng(seed)
    return np.sort(np.concatenate([np.arange(180), rng.integers(0, 180, nlev - 180)]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("padding"), ids=str)
def test_zero_thickness_padding(gpu_ctx, case):
    """A 180-level profile padded to 600 / 1024 levels with repeated levels (dz = 0: zero optical depth) gives the
    256-lane result to 1e-9 K on the tall classes -- the oracle gives it exactly"""
    from oracle import c_oracle as co
    c = case
    base = dataclasses.replace(c, nlev=180)
    P = profiles(180, 160)
    idx = padded_index(c.nlev, c.nlev)
    Q = {k: np.ascontiguousarray(v[:, idx]) for k, v in P.items()}
    frq, ang = FREQS[c.frq], angles(c.nang, low=True)
    kw = opt_inputs_of(c, P, 7)
    kq = {k: np.ascontiguousarray(v[:, idx]) for k, v in kw.items()}
    m = sp.get_model(c.model)
    for i in range(2):
        a, b = (co.tb_profile_opt(m, R["z"][i], R["p"][i], R["t"][i], R["rh"][i], frq, ang,
                                  *(x[k][i] if k in x else None for k in ("denliq", "denice"))) for R, x in ((P, kw), (Q, kq)))
        assert all(np.array_equal(a[k], b[k]) for k in a), "the oracle itself is not padding-invariant"
    if c.entry == "alpha":
        (t0, v0, *_), (t1, v1, *_) = run_alpha(gpu_ctx, base, P, ang), run_alpha(gpu_ctx, c, Q, ang)
        e0 = e1 = None
    else:
        t0, v0, e0 = run_tb(gpu_ctx, base, P, ang, kw)
        t1, v1, e1 = run_tb(gpu_ctx, c, Q, ang, kq)
    family = "padding " + (ALPHA if c.entry == "alpha" else tb_variant(c.options))
    assert (v0 == 1).all() and (v1 == 1).all()
    dev = float(np.abs(t1 - t0).max())
    record(family + " TB", dev)
    assert dev <= 1e-9, dev
    if e0 is not None:
        for k in ("tbatm", "tmr"):
            dev = float(np.abs(e1[k] - e0[k]).max())
            record(f"{family} {k}", dev)
            assert dev <= 1e-9, (k, dev)
        for k in ("tauwet", "taudry", "tauliq", "tauice"):
            assert np.allclose(e1[k], e0[k], rtol=TOL_REL, atol=1e-14), k
            record(f"{family} {k} (rel)", relerr(e1[k][e0[k] > 1e-12], e0[k][e0[k] > 1e-12]))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [TB_ONLY, OPT, FULL, ALPHA])
def test_chunk_widths_agree_on_the_tall_class(gpu_ctx, variant):
    """The same 1024-level call at chunk widths 8, 14 and 16 (5, 3 and 3 chunks of nf = 33): TBs to 1e-8 K (the
    chunk-mate bound of include/mwrt.h), optical depths to 1e-9 relative"""
    group = [c for c in cases_of("widths") if (ALPHA if c.entry == "alpha" else tb_variant(c.options)) == variant]
    assert [c.chunk_width for c in group] == [8, 14, 16]
    P = profiles(1024, 180)
    ang = angles(group[0].nang, low=True)
    kw = opt_inputs_of(group[0], P, 9)
    res = {}
    for c in group:
        if c.entry == "alpha":
            tb, v, *_ = run_alpha(gpu_ctx, c, P, ang)
            res[c.chunk_width] = (tb, v, None)
        else:
            res[c.chunk_width] = run_tb(gpu_ctx, c, P, ang, kw)
    t16, v16, e16 = res[16]
    assert (v16 == 1).all()
    for w in (8, 14):
        tb, v, ex = res[w]
        assert np.array_equal(v, v16)
        dev = float(np.abs(tb - t16).max())
        record(f"widths {variant} TB", dev)
        assert dev <= 1e-8, (w, dev)
        if ex is not None:
            for k in ("tbatm", "tmr"):
                assert np.abs(ex[k] - e16[k]).max() <= 1e-8, (w, k)
            for k in ("tauwet", "taudry", "tauliq", "tauice", "taulay"):
                assert np.allclose(ex[k], e16[k], rtol=TOL_REL, atol=1e-15), (w, k)


@pytest.mark.gpu
def test_remaining_kernels_at_1024_levels(gpu_ctx):
    """k_selftest_math, k_absorb_tl + k_jac_rte (behind the host and the device entry) and k_ray_paths: TBs equal tb_batch's to
    1e-9 K (their exact parity is held in test_gpu_parity / test_jacobian_device_edges)"""
    import torch
    from oracle import c_oracle as co
    misc = {c.entry + ("-rays" if c.options else ""): c for c in cases_of("misc")}
    x = np.array([-600.0, -30.0, -1.0, 0.0, 0.5, 3.0, 700.0])
    y = np.array([1e-300, 0.25, 1.0, 1.0 + 1e-9, 2.0, 1e5, 1e300])
    ex, lg, dv, dv1 = gpu_ctx.selftest_math(x, y)
    assert np.abs(ex / np.exp(x) - 1).max() < 5e-16 and ex[3] == 1.0
    big = np.abs(np.log(y)) > 1e-3
    assert np.abs(lg[big] / np.log(y[big]) - 1).max() < 5e-16 and lg[2] == 0.0
    nz = x != 0
    assert np.abs(dv[nz] * y[nz] / x[nz] - 1).max() < 1e-15 and np.abs(dv1[nz] * y[nz] / x[nz] - 1).max() < 1e-13

    c = misc["jacobian"]
    P = profiles(c.nlev, 200, nprof=1)
    frq, ang = FREQS[c.frq], angles(c.nang)
    ref, rv = gpu_ctx.tb_batch(c.model, P["z"], P["p"], P["t"], P["rh"], frq, ang)
    tb, valid, _ = gpu_ctx.tb_jacobian_batch(c.model, P["z"], P["p"], P["t"], P["rh"], frq, ang)
    assert (valid == 1).all() and (rv == 1).all()
    record("k_jac_rte (host entry) TB vs tb_batch", np.abs(tb - ref).max())
    assert np.abs(tb - ref).max() <= 1e-9

    c = misc["jacobian_device"]                      # same model, profile, frequencies and elevations as the host call
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(P[k]).to(dev) for k in ("z", "p", "t", "rh")}
    out = torch.empty((1, len(ang), len(frq)), dtype=torch.float64, device=dev)
    jac = [torch.empty((1, len(ang), len(frq), c.nlev), dtype=torch.float64, device=dev) for _ in range(3)]
    val = torch.empty(1, dtype=torch.uint8, device=dev)
    gpu_ctx.tb_jacobian_batch_device(c.model, 1, c.nlev, d["z"].data_ptr(), d["p"].data_ptr(), d["t"].data_ptr(),
                                     d["rh"].data_ptr(), frq, ang, out.data_ptr(), *[j.data_ptr() for j in jac], val.data_ptr(),
                                     stream=torch.cuda.current_stream().cuda_stream)
    assert (val.cpu().numpy() == 1).all()
    record("k_jac_rte TB vs tb_batch", np.abs(out.cpu().numpy() - ref).max())
    assert np.abs(out.cpu().numpy() - ref).max() <= 1e-9

    c = misc["tb-rays"]
    frq, ang = FREQS[c.frq], angles(c.nang, low=True)
    tb, valid, _ = run_tb(gpu_ctx, c, P, ang, {"ray_tracing": True})
    r = co.tb_profile_opt(sp.get_model(c.model), P["z"][0], P["p"][0], P["t"][0], P["rh"][0], frq, ang, ray_tracing=True)
    assert valid[0] == 1
    record("rays 1024 TB", np.abs(tb[0].ravel() - r["tbtotal"]).max())
    assert np.abs(tb[0].ravel() - r["tbtotal"]).max() <= TOL_K


@pytest.mark.gpu
def test_helper_selftest_kernels_at_1024_threads(gpu_ctx):
    """the k_selftest_* kernels behind mwrt_selftest_helpers: every selector once in 1024-thread workgroups, two of them with
    the last one partly filled (their accuracy is held in test_math_helpers)"""
    from mwr_fast_forward_operators_and_lbls_amd import _native
    (c,) = cases_of("helpers")
    assert len(expected_kernels(c)) == 8
    n = 2 * 1024 - 100
    x = np.linspace(0.01, 0.1, n)
    for name in _native.HELPERS:
        ins = [np.arange(n) + 0.0, np.full(n, 7.0)] if name == "div_small" else [x, x[::-1].copy(), np.ones(n), x]
        outs, flag = gpu_ctx.selftest_helpers(name, ins, block=1024)
        assert all(np.isfinite(o).all() for o in outs) and not flag.any(), name
        assert np.abs(outs[0]).min() > 0 or name in ("div_small", "block_suffix_excl"), name
    s = gpu_ctx.selftest_helpers("fsqrt", [x], block=1024)[0][0]
    assert np.abs(s * s / x - 1).max() < 1e-13
    v = gpu_ctx.selftest_helpers("layer_value_zf1", [x, x, np.ones(n)], block=1024)[0][0]
    assert np.array_equal(v, x)
    q = gpu_ctx.selftest_helpers("div_small", [np.arange(n) + 0.0, np.full(n, 7.0)], block=1024)[0][0]
    assert np.array_equal(q, np.arange(n) // 7)


@pytest.mark.gpu
def test_lds_budget_as_mirrored(gpu_ctx):
    """The mirror assumes gfx950's 160 KB per workgroup; every case routes the same with the LDS the device reports"""
    import torch
    lds = torch.cuda.get_device_properties(0).shared_memory_per_block
    assert all(route(c, lds) == route(c) for c in CASES), lds
