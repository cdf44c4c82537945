"""Build recipe for libmwrt.so (hipcc, gfx950 only, in-tree so the .so travels with the repo).

Thirteen translation units -- the C-ABI host side (csrc/mwrt.hip, no device code in it), the kernel instantiations of
each frequency-chunk width (csrc/mwrt_inst.hip with -DMWRT_INST_NFC=8|14|16), the device K-matrix kernels
(csrc/mwrt_tl.hip), their ray-traced form (csrc/mwrt_ray.hip), the spectroscopic-parameter Jacobian (csrc/mwrt_par.hip), the optimal-estimation step (csrc/mwrt_oe.hip), its
Levenberg-Marquardt split (csrc/mwrt_oe_lm.hip), its characterisation (csrc/mwrt_oe_char.hip), the instrument
operator (csrc/mwrt_obs.hip), the non-template
kernels (csrc/mwrt_aux.hip) and the host-only launch planning
(csrc/mwrt_plan.cpp, no HIP in it) -- and a fourteenth, the reduced-basis state map (csrc/mwrt_basis.hip), are compiled in
parallel and linked into one shared library; so is a fifteenth, the pre-whitening with a per-profile observation-error
covariance (csrc/mwrt_whiten.hip)."""
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
AUX = os.path.join(CSRC, "mwrt_aux.hip")
PLAN = os.path.join(CSRC, "mwrt_plan.cpp")
# what the library is built from: every file of csrc/ (a new header counts without being named here) and the public header
DEPS = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [os.path.join(ROOT, "include", "mwrt.h")]
LIB = os.path.join(HERE, "libmwrt.so")
OBJ_DIR = os.path.join(HERE, "build")
INST_WIDTHS = (8, 14, 16)


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


def build_native(force: bool = False, verbose: bool = False, extra_flags=(), out: str = None) -> str:
    """Compile the translation units for gfx950 and link libmwrt.so (or ``out``).  Returns the library path."""
    lib = out or LIB
    if not force and out is None and not is_stale():
        return LIB
    hipcc = hipcc_path()
    os.makedirs(OBJ_DIR, exist_ok=True)
    tag = str(os.getpid())
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
              *extra_flags]
    jobs = [(SRC, os.path.join(OBJ_DIR, f"mwrt.{tag}.o"), [])]
    jobs += [(INST, os.path.join(OBJ_DIR, f"mwrt_inst{n}.{tag}.o"), [f"-DMWRT_INST_NFC={n}"]) for n in INST_WIDTHS]
    jobs.append((TL, os.path.join(OBJ_DIR, f"mwrt_tl.{tag}.o"), []))
    jobs.append((RAY, os.path.join(OBJ_DIR, f"mwrt_ray.{tag}.o"), []))
    jobs.append((PAR, os.path.join(OBJ_DIR, f"mwrt_par.{tag}.o"), []))
    jobs.append((OE, os.path.join(OBJ_DIR, f"mwrt_oe.{tag}.o"), []))
    jobs.append((OE_LM, os.path.join(OBJ_DIR, f"mwrt_oe_lm.{tag}.o"), []))
    jobs.append((OE_CHAR, os.path.join(OBJ_DIR, f"mwrt_oe_char.{tag}.o"), []))
    jobs.append((OBS, os.path.join(OBJ_DIR, f"mwrt_obs.{tag}.o"), []))
    jobs.append((BASIS, os.path.join(OBJ_DIR, f"mwrt_basis.{tag}.o"), []))
    jobs.append((WHITEN, os.path.join(OBJ_DIR, f"mwrt_whiten.{tag}.o"), []))
    jobs.append((AUX, os.path.join(OBJ_DIR, f"mwrt_aux.{tag}.o"), []))
    jobs.append((PLAN, os.path.join(OBJ_DIR, f"mwrt_plan.{tag}.o"), []))

    def compile_one(job):
        src, obj, defs = job
        cmd = common + defs + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        return obj

    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
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
