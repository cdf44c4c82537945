"""Holds a kernel trace against the kernel inventory and the routing mirror of tests/test_kernel_instantiations.py.

    python tools/kernel_coverage.py STATS_CSV [LIB]

STATS_CSV is the kernel-stats CSV of ``rocprofv3 --kernel-trace --stats --output-format csv`` over
``pytest tests/test_kernel_instantiations.py -m gpu``; LIB defaults to the in-tree libmwrt.so.  Prints the inventory kernels
the trace never launched and the mwrt kernels it launched that the mirror did not predict; exits 0 only when every
inventory kernel was launched, nothing else was, and the mirror's union over CASES is the inventory."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_kernel_instantiations as ki  # noqa: E402


def traced_kernels(path):
    """mwrt kernel names (normalised) launched in a kernel-stats CSV, with their call counts"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = ki.normalise_kernel_name(row.get("Name") or row.get("name") or "")
            if name:
                out[name] = out.get(name, 0) + int(row.get("Calls") or row.get("total_calls") or 0)
    return out


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    lib = argv[2] if len(argv) > 2 else os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "libmwrt.so")
    inventory = ki.kernel_inventory(lib)
    predicted = set().union(*(ki.expected_kernels(c) for c in ki.CASES))
    traced = traced_kernels(argv[1])
    missing = sorted(inventory - set(traced))
    unpredicted = sorted(set(traced) - predicted)
    mirror_gap = sorted(inventory ^ predicted)
    print(f"inventory {len(inventory)} kernels, predicted {len(predicted)}, launched {len(traced)} "
          f"({sum(traced.values())} launches)")
    for title, names in (("inventory kernels never launched", missing), ("launched but not predicted", unpredicted),
                         ("inventory and mirror differ", mirror_gap)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("  " + n)
    return 0 if not (missing or unpredicted or mirror_gap) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
