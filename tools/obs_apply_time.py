"""Device time of the instrument operator (mwrt_obs_apply_device) next to the routes a user would otherwise
write in torch and to the K-matrix calls around it, one process, one stream, HIP events, at 1000 profiles x 180 levels,
blocks T and humidity, 7 elevations x 3 beam nodes and 14 channels x 3 band nodes (21 x 42 -> 7 x 14):

  (a) obs_apply      mwrt_obs_apply_device: the TB pair and both K blocks
  (b) torch_gather   the gather route on the same buffers: index_select of the referenced rows, multiply by the weights, sum
                     over the node axis (per block, plus the TB vector)
  (c) torch_dense    the dense route: torch.matmul(W, K) with the [98][882] matrix
  (d) kmatrix_grid   the K-matrix call on the 21 x 42 quadrature grid (what the instrument makes the forward model cost)
  (e) kmatrix_centre the K-matrix call on the 7 x 14 centre grid beside it

The five are run alternately, repetition by repetition, each between one pair of HIP events on the current stream.  The file
also holds the bytes (a) must move, computed from the shapes, the resulting GB/s and its share of the 6.29 TB/s a float4 copy
reaches on an MI355X (8.0 TB/s by the data sheet).
Usage: python tools/obs_apply_time.py [--reps N] [--nprof N] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument

HBM_MEASURED_TB_S = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nat.default_context(0)
    nprof, nlev, frq, ang = a.nprof, pr.N_LEVELS, pr.HATPRO_FRQS, pr.BENCH_ELEVATIONS_7
    inst = Instrument(frq, ang, beam=3.5, band=[0.23] * 10 + [0.6, 0.6, 1.0, 2.0], n_beam=3, n_band=3)
    nang_q, nf_q, m_in, m_out = inst.elev_q.size, inst.frq_q.size, inst.m_in, inst.m_out
    assert (nang_q, nf_q, m_out) == (21, 42, 98)
    f64 = dict(dtype=torch.float64, device="cuda")
    P = pr.synthetic_profiles(nprof, 2)
    z, p, t, rh = (torch.tensor(P[k], **f64) for k in ("z", "p", "t", "rh"))
    cur = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    variables = nat.JacVariables.of(humidity="rh")

    def buffers(na, nf):
        return (torch.empty((nprof, na, nf), **f64), torch.empty((nprof, na, nf, nlev), **f64),
                torch.empty((nprof, na, nf, nlev), **f64), torch.empty(nprof, dtype=torch.uint8, device="cuda"))

    tb, k_t, k_h, valid = buffers(nang_q, nf_q)
    tb_c, k_tc, k_hc, valid_c = buffers(ang.size, frq.size)

    def kmatrix(f, e, bufs):
        b_tb, b_t, b_h, b_v = bufs
        ctx.tb_jacobian_batch_vars_device("R24", nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), f, e,
                                          b_tb.data_ptr(), b_t.data_ptr(), b_h.data_ptr(), b_v.data_ptr(),
                                          variables=variables, stream=cur())

    kmatrix(inst.frq_q, inst.elev_q, (tb, k_t, k_h, valid))
    torch.cuda.synchronize()
    _, handle = inst.native_handle(0)
    tb_out = torch.empty((nprof, m_out), **f64)
    k_out = [torch.empty((nprof, m_out, nlev), **f64) for _ in range(2)]
    k_in = [k_t.reshape(nprof, m_in, nlev), k_h.reshape(nprof, m_in, nlev)]
    tb_in = tb.reshape(nprof, m_in)

    def obs_apply():
        ctx.obs_apply_device(handle, nprof, nlev, d_tb_in=tb_in.data_ptr(), d_tb_out=tb_out.data_ptr(),
                             d_k_in=[k.data_ptr() for k in k_in], d_k_out=[k.data_ptr() for k in k_out], stream=cur())

    # the gather route: every row has the same number of entries here (3 x 3), so the entries form a [m_out][9] table
    nnz = np.diff(inst.row_ptr)
    assert (nnz == nnz[0]).all()
    col = torch.tensor(inst.col.astype(np.int64), device="cuda")
    wts = torch.tensor(inst.w, **f64).reshape(1, m_out, int(nnz[0]))
    dense = torch.tensor(inst.dense(), **f64)
    held = {}

    def torch_gather():
        held["g_tb"] = (tb_in.index_select(1, col).reshape(nprof, m_out, -1) * wts).sum(dim=2)
        held["g_k"] = [(k.index_select(1, col).reshape(nprof, m_out, -1, nlev) * wts[..., None]).sum(dim=2) for k in k_in]

    def torch_dense():
        held["d_tb"] = torch.matmul(tb_in, dense.T)
        held["d_k"] = [torch.matmul(dense, k) for k in k_in]

    paths = (("obs_apply", obs_apply), ("torch_gather", torch_gather), ("torch_dense", torch_dense),
             ("kmatrix_grid", lambda: kmatrix(inst.frq_q, inst.elev_q, (tb, k_t, k_h, valid))),
             ("kmatrix_centre", lambda: kmatrix(frq, ang, (tb_c, k_tc, k_hc, valid_c))))
    for _ in range(3):
        for _, fn in paths:
            fn()                                               # warm-up: code objects, small copies, torch's allocator
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in paths}
    for _ in range(a.reps):
        for name, fn in paths:                                 # alternately, in the same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"shape": {"nprof": nprof, "nlev": nlev, "nblk": 2, "nang_q": nang_q, "nf_q": nf_q, "m_in": m_in, "m_out": m_out,
                     "nnz_per_row": int(nnz[0]), "model": "R24"}, "reps": a.reps,
           "double2_variant": "tried (two levels per lane for even nlev) and not kept: 0.575 against 0.569 ms, DESIGN 4.7"}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    torch.cuda.synchronize()
    scale = max(float(held["g_k"][0].abs().max()), 1e-300)
    res["largest_difference_vs_torch_gather_of_max_abs"] = float((k_out[0] - held["g_k"][0]).abs().max() / scale)
    res["largest_difference_vs_torch_dense_of_max_abs"] = float((k_out[0] - held["d_k"][0]).abs().max() / scale)
    res["largest_tb_difference_vs_torch_gather_K"] = float((tb_out - held["g_tb"]).abs().max())
    med = lambda k: res[k]["median_ms"]   # noqa: E731
    moved = 2 * nprof * (m_in + m_out) * nlev * 8 + nprof * (m_in + m_out) * 8
    res["obs_apply_bytes"] = moved
    res["obs_apply_gb_per_s"] = moved / (med("obs_apply") * 1e-3) / 1e9
    res["obs_apply_share_of_measured_hbm_peak"] = res["obs_apply_gb_per_s"] / (HBM_MEASURED_TB_S * 1e3)
    res["hbm_measured_peak_tb_per_s"] = HBM_MEASURED_TB_S
    res["ratio_obs_apply_over_torch_gather"] = med("obs_apply") / med("torch_gather")
    res["ratio_obs_apply_over_torch_dense"] = med("obs_apply") / med("torch_dense")
    res["ratio_kmatrix_grid_over_centre"] = med("kmatrix_grid") / med("kmatrix_centre")
    # the expectation: (a) no slower than (b) beyond the overlap of their p10-p90 bands
    res["obs_apply_no_slower_than_torch_gather"] = bool(res["obs_apply"]["p10_ms"] <= res["torch_gather"]["p90_ms"])
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    inst.close()


if __name__ == "__main__":
    main()
