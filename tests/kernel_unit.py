"""What the tests of a kernel unit ask without a GPU, once for all units (a plain module, imported like the *_reference
ones): the compiler's resource remark for a unit compiled by the library's own command, the kernels of the built library by
namespace, the fields of a record of include/mwrt.h against its ctypes mirror, and the values of a plan header."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

from mwr_fast_forward_operators_and_lbls_amd import build

MWRT_H = os.path.join(build.ROOT, "include", "mwrt.h")
# a demangled kernel, as nm -C and c++filt print it: mwrt::[namespace::][(anonymous namespace)::]k_name[<arguments>](
_KERNEL = re.compile(r"(?:^|\s)mwrt::((?:\w+::)*)(?:\(anonymous namespace\)::)?(k_\w+(?:<[^>()]*>)?)\(")
_REMARK = re.compile(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)")


@functools.lru_cache(maxsize=None)
def resource_usage(src, defs=()):
    """{kernel as nm -C names it: {"VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS"}} from the resource remark of `src`
    compiled for gfx950 by build.compile_command with `defs`.  One compile per (src, defs) and process; do not change it."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = build.compile_command(src, os.path.join(tmp, "unit.o"), defs) + ["-Rpass-analysis=kernel-resource-usage"]
        remarks = _REMARK.findall(subprocess.run(cmd, check=True, capture_output=True, text=True).stderr)
    mangled = [value for key, value in remarks if key == "Function Name"]
    plain = subprocess.run(["c++filt"], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(plain) == len(mangled)
    names = {}                                                           # a function that is no kernel keeps its full name
    for m, p in zip(mangled, plain):
        kernel = _KERNEL.search(p)
        names[m] = kernel.group(2) if kernel else p
    out, name = {}, None
    for key, value in remarks:
        if key == "Function Name":
            name = names[value]
            assert name not in out, name
            out[name] = {}
        else:
            out[name][key.split(" ")[0]] = int(value)
    assert all(set(u) == {"VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS"} for u in out.values()), out
    return out


@functools.lru_cache(maxsize=None)
def library_kernels(lib_path):
    """{namespace under mwrt ("" for mwrt itself): the kernels compiled into `lib_path`}: the host handles, anonymous-namespace
    ones included, the __device_stub__ symbols beside them skipped."""
    out = {}
    for line in subprocess.run(["nm", "-C", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout.splitlines():
        m = None if "__device_stub__" in line else _KERNEL.search(line)
        if m:
            out.setdefault(m.group(1)[:-2], set()).add(m.group(2))
    return out


def record_field_names(record):
    """The field names of `typedef struct <record>` in include/mwrt.h, in order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (record, record), open(MWRT_H).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]


def check_record(native_lib, record, mirror, size, names=None, offsets=None):
    """The record in the header, field by field and in order, is the ctypes `mirror`; <record>_size() and the mirror are `size`
    bytes; `names` and `offsets` (of every field) are what the unit pins beside that.  Returns the names."""
    got = record_field_names(record)
    assert got == [f[0] for f in mirror._fields_], got
    assert names is None or got == names, got
    assert getattr(native_lib, record + "_size")() == ctypes.sizeof(mirror) == size
    assert offsets is None or [getattr(mirror, n).offset for n in got] == offsets
    return got


def plan_rows(header, loop_body, tmp_path):
    """The plans of a unit's header are host and device code alike: a host program that runs `loop_body` (C++ that prints one
    line of integers) for n = 1 .. MWRT_OE_NFORM_MAX_N is compiled here with hipcc and run.  Returns the lines as tuples."""
    src, exe = tmp_path / "plans.hip", str(tmp_path / "plans")
    src.write_text('#include <cstdio>\n#include "%s"\nint main() {\n  for (int n = 1; n <= MWRT_OE_NFORM_MAX_N; ++n) {\n%s\n  }\n'
                   '  return 0;\n}\n' % (header, loop_body))
    subprocess.run([build.hipcc_path(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(build.ROOT, "include"),
                    str(src), "-o", exe], check=True, capture_output=True)
    return [tuple(map(int, ln.split())) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
