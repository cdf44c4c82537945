"""Build recipe for libmwrt.so (hipcc, gfx950 only, in-tree so the .so travels with the repo).

UNITS lists the translation units, each a source of csrc/ with the defines it is compiled under: the two C-ABI host units
(mwrt.hip and mwrt_retrieval.hip, no device code in either), one kernel unit per stage (mwrt_inst.hip once per
frequency-chunk width), and the host-only planning and argument stage (mwrt_plan.cpp and mwrt_records.cpp, no HIP in
them).  They are compiled in parallel and linked into one shared library."""
from __future__ import annotations

import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SRC = os.path.join(CSRC, "mwrt.hip")
INST = os.path.join(CSRC, "mwrt_inst.hip")
TL = os.path.join(CSRC, "mwrt_tl.hip")
RAY = os.path.join(CSRC, "mwrt_ray.hip")
PAR = os.path.join(CSRC, "mwrt_par.hip")
OE = os.path.join(CSRC, "mwrt_oe.hip")
OE_LM = os.path.join(CSRC, "mwrt_oe_lm.hip")
OE_CHAR = os.path.join(CSRC, "mwrt_oe_char.hip")
OBS = os.path.join(CSRC, "mwrt_obs.hip")
BASIS = os.path.join(CSRC, "mwrt_basis.hip")
WHITEN = os.path.join(CSRC, "mwrt_whiten.hip")
NFORM = os.path.join(CSRC, "mwrt_nform.hip")
NFORM_CHAR = os.path.join(CSRC, "mwrt_nform_char.hip")
SELECT = os.path.join(CSRC, "mwrt_select.hip")
AUX = os.path.join(CSRC, "mwrt_aux.hip")
PLAN = os.path.join(CSRC, "mwrt_plan.cpp")
RETRIEVAL = os.path.join(CSRC, "mwrt_retrieval.hip")
RECORDS = os.path.join(CSRC, "mwrt_records.cpp")
INST_WIDTHS = (8, 14, 16)
#: the translation units of the library: (source, extra defines)
UNITS = [(SRC, []), (RETRIEVAL, [])] + [(INST, [f"-DMWRT_INST_NFC={n}"]) for n in INST_WIDTHS] + [
    (unit, []) for unit in (TL, RAY, PAR, OE, OE_LM, OE_CHAR, OBS, BASIS, WHITEN, NFORM, NFORM_CHAR, SELECT, AUX, PLAN, RECORDS)]
#: the units that hold the C entry points: host code only
HOST_UNITS = (SRC, RETRIEVAL)
MAX_COMPILE_WORKERS = 16
# what the library is built from: every file of csrc/ (a new header counts without being named here) and the public header
DEPS = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [os.path.join(ROOT, "include", "mwrt.h")]
LIB = os.path.join(HERE, "libmwrt.so")
OBJ_DIR = os.path.join(HERE, "build")


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm; no other compiler can build the gfx950 kernels)")


def is_stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in DEPS)


def compile_command(src: str, obj: str, defs=(), extra=()) -> list:
    """The command that compiles one translation unit of the library, a row of UNITS, for gfx950 into ``obj``."""
    return [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
            *extra, *defs, "-c", src, "-o", obj]


def build_native(force: bool = False, verbose: bool = False, extra_flags=(), out: str = None) -> str:
    """Compile the translation units for gfx950 and link libmwrt.so (or ``out``).  Returns the library path."""
    lib = out or LIB
    if not force and out is None and not is_stale():
        return LIB
    hipcc = hipcc_path()
    os.makedirs(OBJ_DIR, exist_ok=True)
    tag = str(os.getpid())
    jobs = [(src, os.path.join(OBJ_DIR, f"{os.path.splitext(os.path.basename(src))[0]}.{i}.{tag}.o"), defs)
            for i, (src, defs) in enumerate(UNITS)]

    def compile_one(job):
        src, obj, defs = job
        cmd = compile_command(src, obj, defs, extra_flags)
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        return obj

    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(jobs), MAX_COMPILE_WORKERS, os.cpu_count() or 1)) as pool:
            objs = list(pool.map(compile_one, jobs))
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib + ".tmp", *objs]
        if verbose:
            print(" ".join(link), file=sys.stderr)
        subprocess.run(link, check=True)
        os.replace(lib + ".tmp", lib)
    finally:
        for _, obj, _ in jobs:
            if os.path.exists(obj):
                os.remove(obj)
    return lib


if __name__ == "__main__":
    print(build_native(force="--force" in sys.argv, verbose=True))
