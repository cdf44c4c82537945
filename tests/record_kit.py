"""What the tests/test_*record_checks.py share: the ``record_dump`` fixture -- tests/record_dump.cpp linked with
csrc/mwrt_records.cpp as is, built with the host C++ compiler under ASan + UBSan, once per session, and run as a program of
its own -- and the helpers that build records from the ctypes mirrors of _native.py and hold the answers against a case
list.  Test modules import the fixture from here (``from record_kit import record_dump``)."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")
OK, INVALID, UNSUPPORTED = 0, -1, -5                 # include/mwrt.h mwrt_status
_EXE = {}


@pytest.fixture(scope="module")
def record_dump(tmp_path_factory):
    """ask(request lines) -> one parsed JSON answer per line.  A sanitiser report ends the child with a non-zero status."""
    if "exe" not in _EXE:
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        exe = str(tmp_path_factory.mktemp("record_dump") / "record_dump")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "record_dump.cpp"), os.path.join(CSRC, "mwrt_records.cpp"), "-o", exe], check=True)
        _EXE["exe"] = exe

    def ask(lines):
        r = subprocess.run([_EXE["exe"]], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


def leaves(cls):
    """(name, element index or None, offset, size) of every field, an array counted element by element."""
    out = []
    for name, kind in cls._fields_:
        off = getattr(cls, name).offset
        if issubclass(kind, ctypes.Array):
            out += [(name, i, off + i * ctypes.sizeof(kind._type_), ctypes.sizeof(kind._type_)) for i in range(kind._length_)]
        else:
            out.append((name, None, off, ctypes.sizeof(kind)))
    return out


def put(rec, name, index, value):
    if index is None:
        setattr(rec, name, value)
    else:
        getattr(rec, name)[index] = value


def record(cls, struct_size=None, **fields):
    """A record every entry of its family accepts: every pointer given and distinct (0x1000 + its offset), every integer 0
    but nblk = 1, struct_size = sizeof; then `fields` (an array element as name_i=value, None for a NULL pointer)."""
    rec = cls()
    for name, index, off, _ in leaves(cls):
        if name.startswith("d_"):
            put(rec, name, index, 0x1000 + off)
    rec.struct_size = ctypes.sizeof(cls) if struct_size is None else struct_size
    if hasattr(rec, "nblk"):
        rec.nblk = 1
    for key, value in fields.items():
        name, _, index = key.rpartition("_") if key[-1].isdigit() and key[-2] == "_" else (key, "", None)
        put(rec, name, None if index is None else int(index), value)
    return rec


def line(entry, *scalars_and_record):
    *scalars, rec = scalars_and_record
    return " ".join([entry, *map(str, scalars), bytes(rec).hex()])


def run(record_dump, cases):
    """cases: (request line, status, message or None for 'accepted'[, record that comes out])"""
    got = record_dump([c[0] for c in cases])
    for case, g in zip(cases, got):
        request, status, message = case[:3]
        assert (g["status"], g["message"]) == (status, message or ""), request[:60]
        if len(case) > 3:
            assert g["record"] == bytes(case[3]).hex(), request[:60]
