"""Wall time of the batched K-matrix entry on host buffers (mwrt_tb_jacobian_batch: the device K-matrix, k_absorb_tl +
k_jac_rte, behind a staging copy) next to the forward call.  The device work is well under a millisecond (0.58 ms at 1000
profiles x 14 channels x 7 elevations); the rest is the partial derivatives (60 MB per elevation at 1000
profiles) crossing PCIe into pageable memory.  Record: profiles/jacobian_host_entry_time.json."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mwr_fast_forward_operators_and_lbls_amd import _native as nat, profiles as pr
ctx = nat.Context(0)
for nprof, ang in ((100, np.array([90.0])), (1000, np.array([90.0])), (1000, pr.BENCH_ELEVATIONS_7)):
    P = pr.synthetic_profiles(nprof, 5)
    r = ctx.tb_jacobian_batch("R24", P["z"], P["p"], P["t"], P["rh"], pr.HATPRO_FRQS, ang)
    t0 = time.perf_counter()
    for _ in range(3):
        r = ctx.tb_jacobian_batch("R24", P["z"], P["p"], P["t"], P["rh"], pr.HATPRO_FRQS, ang)
    dt = (time.perf_counter() - t0) / 3
    t0 = time.perf_counter()
    for _ in range(3):
        ctx.tb_batch("R24", P["z"], P["p"], P["t"], P["rh"], pr.HATPRO_FRQS, ang)
    dt2 = (time.perf_counter() - t0) / 3
    print(f"nprof={nprof} nang={len(ang)}: K-matrix call {dt*1e3:.2f} ms (host buffers; outputs {sum(np.asarray(x).nbytes for x in r if hasattr(x,'nbytes'))/1e6:.0f} MB), forward call {dt2*1e3:.2f} ms")
