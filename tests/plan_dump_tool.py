"""The ``plan_dump`` fixture: tests/plan_dump.cpp linked with csrc/mwrt_plan.cpp as is, built with the host C++ compiler
under ASan + UBSan and run as a program of its own.  Test modules import the fixture from here
(``from plan_dump_tool import plan_dump``); the program is built once per session.  ``plan_dump_plain`` is the same
program without the sanitisers, for the GPU tests."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")
_EXE = {}


def request(*a):
    """one request line: floats in their shortest round-trip form"""
    return " ".join(repr(float(x)) if isinstance(x, (float, np.floating)) else str(x) for x in a)


def build(directory, sanitise=True):
    """compile the program into `directory` -> its path"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), "plan_dump")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitise else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, os.path.join(ROOT, "tests", "plan_dump.cpp"), os.path.join(CSRC, "mwrt_plan.cpp"), "-o", exe], check=True)
    return exe


def asker(exe):
    """-> ask(request lines) -> one parsed JSON answer per line.  A sanitiser report ends the child with a non-zero status."""
    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """ask(request lines) of the sanitised program"""
    if "exe" not in _EXE:
        _EXE["exe"] = build(tmp_path_factory.mktemp("plan_dump"))
    return asker(_EXE["exe"])


@pytest.fixture(scope="module")
def plan_dump_plain(tmp_path_factory):
    """the same program built without the sanitisers, for the tests that run next to a GPU (sanitised runs stay on the CPU side)"""
    if "plain" not in _EXE:
        _EXE["plain"] = build(tmp_path_factory.mktemp("plan_dump_plain"), sanitise=False)
    return asker(_EXE["plain"])
