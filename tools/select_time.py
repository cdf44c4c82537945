"""Device time of the observation selection (mwrt_oe_select_device) beside the same algorithm written in torch
on the same buffers: one process, one stream, HIP events.  1000 profiles of a synthetic K B of the statistics of a projected
K-matrix (rows of a few strong directions plus noise), at (r, m, nsel) = (24, 224, 98), (32, 98, 98) and (64, 896, 64): one
block of r coefficients, S0 = diag of a decaying spectrum, shared variances.

  select_rR_mM_sS          mwrt_oe_select_device with d_dfs_gain, d_post_cov and d_post_var
  select_plain_rR_mM_sS    ... the required outputs alone
  torch_rR_mM_sS           the same incremental algorithm in torch: per round one argmax, two gathers, one bmv, one rank-one
                           update of S and one einsum over K, with the same stop rule and the same outputs
``k_bytes_per_round`` is what one pass over K moves (nprof m r doubles); ``k_gb_s`` that times nsel + 1 over the kernel's
time, against ``copy``: torch's device-to-device copy of a 1 GiB float64 buffer, 2 GiB moved per call, interleaved with the
other paths.  ``check_*`` holds whether the two paths picked the same order and the largest differences of q and post_cov,
so a baseline that computes something else shows.

All paths are run alternately, repetition by repetition, each between one pair of HIP events on the current stream.  Median
[p10 - p90] of ``--reps`` repetitions after warm-up.  Usage: python tools/select_time.py [--reps N] [--nprof N] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat

COPY_BYTES = 1 << 30
SHAPES = ((24, 224, 98), (32, 98, 98), (64, 896, 64))


def torch_select(k, se, s0, sa_inv, nsel):
    """The incremental form of include/mwrt.h on [nprof][m][r] in torch -> order, q_pick, dfs_gain, S, q."""
    nprof, m, r = k.shape
    s = s0.expand(nprof, r, r).clone()
    q = torch.einsum("pmi,pij,pmj->pm", k, s, k) / se
    free = torch.ones((nprof, m), dtype=torch.bool, device=k.device)
    order = torch.full((nprof, nsel), -1, dtype=torch.int64, device=k.device)
    q_pick = torch.zeros((nprof, nsel), dtype=torch.float64, device=k.device)
    dfs = torch.zeros((nprof, nsel), dtype=torch.float64, device=k.device)
    rows = torch.arange(nprof, device=k.device)
    for t in range(nsel):
        best, j = torch.where(free, q, torch.full_like(q, -1.0)).max(dim=1)
        go = best > 0
        kj = k[rows, j]
        v = torch.bmm(s, kj.unsqueeze(2)).squeeze(2)
        d = se[j] + (kj * v).sum(dim=1)
        order[:, t] = torch.where(go, j, torch.full_like(j, -1))
        q_pick[:, t] = torch.where(go, best, torch.zeros_like(best))
        dfs[:, t] = torch.where(go, ((v @ sa_inv) * v).sum(dim=1) / d, torch.zeros_like(d))
        scale = torch.where(go, 1.0 / d, torch.zeros_like(d))
        s = s - scale[:, None, None] * v[:, :, None] * v[:, None, :]
        free[rows, j] = free[rows, j] & ~go
        kv = torch.einsum("pmi,pi->pm", k, v)
        q = torch.where(free, torch.clamp(q - scale[:, None] * kv * kv / se, min=0.0), q)
    return order, q_pick, dfs, s, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)                                # no GPU: this raises, and so does the first CUDA tensor
    nprof = a.nprof
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    gen = torch.Generator(device="cuda").manual_seed(2100)
    paths, cases, held = [], {}, {}
    for r, m, nsel in SHAPES:
        lam = 4.0 * torch.exp(-torch.arange(r, **f64) / (r / 6.0))
        s0 = torch.diag(lam).contiguous()
        sa_inv = torch.diag(1.0 / lam).contiguous()
        amp = torch.rand((nprof, m, 1), generator=gen, **f64) * 0.8 + 0.2
        k = (amp * torch.randn((nprof, m, r), generator=gen, **f64) * torch.exp(-torch.arange(r, **f64) / (r / 3.0))).contiguous()
        se = torch.full((m,), 0.25, **f64)
        q = dict(k=k, se=se, s0=s0, sa_inv=sa_inv, r=r, m=m, nsel=nsel,
                 order=torch.empty((nprof, nsel), **i32), q_pick=torch.empty((nprof, nsel), **f64), rank=torch.empty((nprof, m), **i32),
                 q=torch.empty((nprof, m), **f64), count=torch.empty(nprof, **i32), status=torch.empty(nprof, dtype=torch.uint8, device="cuda"),
                 dfs_gain=torch.empty((nprof, nsel), **f64), post_cov=torch.empty((nprof, r, r), **f64), post_var=torch.empty((nprof, 1, r), **f64))
        tag = f"r{r}_m{m}_s{nsel}"
        cases[tag] = q

        def select(q=q, every=True):
            opt = dict(d_sa_inv=q["sa_inv"].data_ptr(), d_dfs_gain=q["dfs_gain"].data_ptr(), d_post_cov=q["post_cov"].data_ptr(),
                       d_post_var=q["post_var"].data_ptr()) if every else {}
            ctx.oe_select_device(nprof, q["r"], q["m"], [q["k"].data_ptr()], q["s0"].data_ptr(), q["se"].data_ptr(), q["nsel"],
                                 q["order"].data_ptr(), q["q_pick"].data_ptr(), q["rank"].data_ptr(), q["q"].data_ptr(),
                                 q["count"].data_ptr(), q["status"].data_ptr(), stream=cur(), **opt)

        def in_torch(q=q, tag=tag):
            held[tag] = torch_select(q["k"], q["se"], q["s0"], q["sa_inv"], q["nsel"])

        paths += [(f"select_plain_{tag}", lambda select=select: select(every=False)), (f"select_{tag}", select),
                  (f"torch_{tag}", in_torch)]
    src = torch.empty(COPY_BYTES // 8, **f64).normal_()
    dst = torch.empty_like(src)
    paths.append(("copy", lambda: dst.copy_(src)))

    for _ in range(2):
        for _, fn in paths:
            fn()                                                # warm-up: code objects, LDS limits, torch's allocator
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in paths}
    for _ in range(a.reps):
        for name, fn in paths:                                  # alternately, in the same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"shape": {"nprof": nprof, "r_m_nsel": [list(s) for s in SHAPES]}, "reps": a.reps}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
    copy_tb_s = 2.0 * COPY_BYTES / (res["copy"]["median_ms"] * 1e-3) / 1e12
    res["copy"].update(bytes_moved=2.0 * COPY_BYTES, tb_s=copy_tb_s)
    norm = lambda v: float(v.abs().amax())                      # noqa: E731
    for tag, q in cases.items():
        order, q_pick, dfs, s, q_left = held[tag]
        torch.cuda.synchronize()
        per_round = 8.0 * nprof * q["m"] * q["r"]
        sec = res[f"select_{tag}"]["median_ms"] * 1e-3
        res[f"summary_{tag}"] = {
            "select_ms": res[f"select_{tag}"]["median_ms"], "torch_ms": res[f"torch_{tag}"]["median_ms"],
            "ratio_select_over_torch": res[f"select_{tag}"]["median_ms"] / res[f"torch_{tag}"]["median_ms"],
            "k_bytes_per_round": per_round, "k_gb_s": per_round * (q["nsel"] + 1) / sec / 1e9,
            "share_of_copy_rate": per_round * (q["nsel"] + 1) / sec / (copy_tb_s * 1e12)}
        res[f"check_{tag}"] = {
            "status_all_1": bool((q["status"] == 1).all()),
            "profiles_with_the_same_order": int((order == q["order"].long()).all(dim=1).sum()),
            "q_pick_over_largest": norm(q_pick - q["q_pick"]) / norm(q["q_pick"]),
            "dfs_gain_over_largest": norm(dfs - q["dfs_gain"]) / norm(q["dfs_gain"]),
            "post_cov_over_largest": norm(s - q["post_cov"]) / norm(q["post_cov"]),
            "q_left_over_largest": norm(q_left - q["q"]) / norm(q["q"])}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
