#!/usr/bin/env python3
"""Per-basic-block and per-source-line instruction table of one kernel, from hipcc --save-temps ISA.

    hipcc --offload-arch=gfx950 -O3 -gline-tables-only --save-temps ... -DMWRT_INST_NFC=14 -c csrc/mwrt_inst.hip
    python tools/isa_blocks.py mwrt_inst-hip-amdgcn-amd-amdhsa-gfx950.s k_tb_fusedILi14ELi7ELi256E [--lines | --loops]

--loops sums the blocks of each loop (the compiler's own "in Loop: Header=" comments; a block counts for its innermost
loop only, "straight" is the code outside every loop) and adds an `arith` column (fma64 + mul64 + add64 + rcp64): what is
left of VALU after it is moves, selects, compares, conversions and lane traffic.

(the unit that holds the kernel: csrc/mwrt_inst.hip for k_tb_fused, k_absorb* and k_rte_tau, csrc/mwrt_tl.hip for the
K-matrix kernels, csrc/mwrt_aux.hip for the rest; csrc/mwrt.hip is host code only)

Static counts only: multiply a loop block by its trip count (O2 line loop = n_o2, H2O = n_h2o ...)
to estimate the dynamic VALU instructions per wave that SQ_INSTS_VALU reports.
"""
from __future__ import annotations

import collections
import re
import sys

CATS = ("valu", "fma64", "mul64", "add64", "rcp64", "lane", "mov", "cnd", "cmp", "salu", "smem", "lds", "vmem")


def classify(op: str):
    c = []
    if op.startswith("v_"):
        c.append("valu")
        if op in ("v_fma_f64", "v_fmac_f64"):
            c.append("fma64")
        elif op == "v_mul_f64":
            c.append("mul64")
        elif op == "v_add_f64":
            c.append("add64")
        elif op in ("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64"):
            c.append("rcp64")
        elif op in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32"):
            c.append("lane")
        elif op.startswith("v_mov") or op.startswith("v_accvgpr"):
            c.append("mov")
        elif op.startswith("v_cndmask"):
            c.append("cnd")
        elif op.startswith("v_cmp"):
            c.append("cmp")
    elif op.startswith("s_load") or op.startswith("s_buffer_load"):
        c.append("smem")
    elif op.startswith("s_"):
        c.append("salu")
    elif op.startswith("ds_"):
        c.append("lds")
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        c.append("vmem")
    return c


def main():
    path, key = sys.argv[1], sys.argv[2]
    by_line = "--lines" in sys.argv
    by_loop = "--loops" in sys.argv
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and key in l and l.rstrip().split(":")[0].endswith("E"))
    blocks, order = collections.defaultdict(collections.Counter), []
    srcs = collections.defaultdict(collections.Counter)
    blk_src = collections.defaultdict(collections.Counter)
    cur, loc = "entry", 0
    order.append(cur)
    loop_of, depth_of, parent_of = {}, {}, {}          # block -> innermost loop header; header -> depth, parent header
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            cur = m.group(1)
            order.append(cur)
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
            if h:
                loop_of[cur] = ".L" + h.group(1)
            for par in re.finditer(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", s):
                parent_of[cur] = ".L" + par.group(1)
            h = re.search(r"Loop Header: Depth=(\d+)", s)
            if h:
                loop_of[cur], depth_of[cur] = cur, int(h.group(1))
            continue
        h = re.search(r"Loop Header: Depth=(\d+)", s)
        if h and s.startswith(";"):
            loop_of[cur] = cur
            depth_of[cur] = int(h.group(1))
            continue
        par = re.search(r"^;\s+Parent Loop (BB\d+_\d+) Depth=(\d+)", s)
        if par:
            parent_of[cur] = ".L" + par.group(1)                # the last one listed is the innermost parent
            continue
        m = re.match(r"^\.loc\s+\d+\s+(\d+)", s)
        if m:
            loc = int(m.group(1))
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", s.split()[0])
        for c in classify(op):
            blocks[cur][c] += 1
            srcs[loc][c] += 1
        if op.startswith("v_"):
            blk_src[cur][loc] += 1
        if op.startswith(("s_cbranch", "s_branch")):
            blocks[cur]["->" + s.split()[-1]] += 1
    hdr = f"{'block':>12} " + " ".join(f"{c:>6}" for c in CATS) + "  top source lines (VALU) / branches"
    if by_loop:
        cols = ("valu", "arith", "mov", "cnd", "cmp", "lane", "salu", "smem", "lds", "vmem")
        loops, lsrc = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
        for b in order:
            key = loop_of.get(b, "straight")
            loops[key].update({c: blocks[b][c] for c in CATS})
            lsrc[key].update(blk_src[b])
        print(f"{'loop':>12} {'depth':>5} {'parent':>12} " + " ".join(f"{c:>6}" for c in cols) + "  top source lines (VALU)")
        for key in ["straight"] + [b for b in order if b in loops]:
            cnt = loops[key]
            cnt["arith"] = cnt["fma64"] + cnt["mul64"] + cnt["add64"] + cnt["rcp64"]
            top = ", ".join(f"{ln}:{n}" for ln, n in lsrc[key].most_common(4))
            print(f"{key:>12} {depth_of.get(key, 0):>5} {parent_of.get(key, '-'):>12} " + " ".join(f"{cnt[c]:>6}" for c in cols) + f"  {top}")
    elif by_line:
        print(f"{'line':>6} " + " ".join(f"{c:>6}" for c in CATS))
        for ln in sorted(srcs):
            if srcs[ln]["valu"]:
                print(f"{ln:>6} " + " ".join(f"{srcs[ln][c]:>6}" for c in CATS))
    else:
        print(hdr)
        tot = collections.Counter()
        for b in order:
            cnt = blocks[b]
            if not any(cnt[c] for c in CATS):
                continue
            tot.update({c: cnt[c] for c in CATS})
            top = ", ".join(f"{ln}:{n}" for ln, n in blk_src[b].most_common(4))
            br = " ".join(k for k in cnt if k.startswith("->"))
            print(f"{b:>12} " + " ".join(f"{cnt[c]:>6}" for c in CATS) + f"  {top}  {br}")
        print(f"{'TOTAL':>12} " + " ".join(f"{tot[c]:>6}" for c in CATS))


if __name__ == "__main__":
    main()
