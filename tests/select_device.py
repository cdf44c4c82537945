"""mwrt_oe_select_device driven on the device for a case of tests/select_reference.py: what tests/test_oe_select.py and
tools/select_errors.py share.  ``SelDev`` holds a case in HBM with sentinel-filled outputs (NaN in the floating-point ones,
-7 in the integers, 9 in the status) so an entry the kernel leaves unwritten shows.  Needs torch with a GPU; a helper, not a
test module."""
import numpy as np
import torch

import select_reference as sr

OPTIONAL = ("dfs_gain", "post_cov", "post_var")
OUT_KEYS = ("order", "q_pick", "rank", "q", "count", "status") + OPTIONAL


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


class SelDev:
    def __init__(self, case, nsel, keep=None, candidate=None, active=None):
        self.k = [_dev(b) for b in case["k"]]
        self.nprof, self.m, self.nlev = self.k[0].shape
        self.nblk, self.nsel = len(self.k), int(nsel)
        self.n = self.nblk * self.nlev
        self.s0, self.se, self.sa_inv = _dev(case["s0"]), _dev(case["se"]), _dev(case["sa_inv"])
        self.s0_pp, self.se_pp = case["s0"].ndim == 3, case["se"].ndim == 2
        self.keep = None if keep is None else _dev(np.asarray(keep, dtype=np.uint8))
        self.candidate = None if candidate is None else _dev(np.asarray(candidate, dtype=np.uint8))
        self.active = None if active is None else _dev(np.asarray(active, dtype=np.uint8))
        self.reset()

    def reset(self):
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        nprof, m, n, nsel = self.nprof, self.m, self.n, self.nsel
        nan = float("nan")
        self.out = dict(order=torch.full((nprof, nsel), -7, **i32), q_pick=torch.full((nprof, nsel), nan, **f64),
                        rank=torch.full((nprof, m), -7, **i32), q=torch.full((nprof, m), nan, **f64),
                        count=torch.full((nprof,), -7, **i32), status=torch.full((nprof,), 9, dtype=torch.uint8, device="cuda"),
                        dfs_gain=torch.full((nprof, nsel), nan, **f64), post_cov=torch.full((nprof, n, n), nan, **f64),
                        post_var=torch.full((nprof, self.nblk, self.nlev), nan, **f64))

    def args(self, outputs=OPTIONAL):
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, d_k=[b.data_ptr() for b in self.k], d_s0=self.s0.data_ptr(),
                    d_se=self.se.data_ptr(), nsel=self.nsel, d_sa_inv=self.sa_inv.data_ptr(), d_keep=ptr(self.keep),
                    d_candidate=ptr(self.candidate), d_active=ptr(self.active), se_per_profile=self.se_pp,
                    s0_per_profile=self.s0_pp, stream=_cur(),
                    **{"d_" + key: self.out[key].data_ptr() for key in OUT_KEYS if key not in OPTIONAL or key in outputs})

    def select(self, ctx, outputs=OPTIONAL):
        ctx.oe_select_device(**self.args(outputs))
        torch.cuda.synchronize()
        return self.host()

    def host(self):
        return {key: v.cpu().numpy() for key, v in self.out.items()}


def profile(got, i):
    """Profile i of a ``host()`` dict."""
    return {key: v[i] for key, v in got.items()}


def judge(case, got, greedy, nsel, keep=None, candidate=None, label=""):
    """Every profile of a device result against the replay of its own order and against the greedy reference: the largest
    error per output in units of the bars (select_reference.select_errors), after asserting status, count, rank, that no
    pick gave up more than 1e-9 of the best and that the order IS the greedy one."""
    n = case["k"][0].shape[2] * len(case["k"])
    worst = {}
    for i, ref in enumerate(greedy):
        g = profile(got, i)
        assert g["status"] == ref["status"], (label, i, g["status"], ref["status"])
        if ref["status"] in (0, 2):
            assert g["count"] == 0 and (g["order"] == -1).all() and (g["rank"] == -1).all(), (label, i)
            for key in ("q_pick", "q", "dfs_gain", "post_cov", "post_var"):
                assert np.isnan(g[key]).all(), (label, i, key)
            continue
        s0 = case["s0"][i] if case["s0"].ndim == 3 else case["s0"]
        rep = sr.replay(case, i, g["order"], ref, None if keep is None else keep, candidate)
        picked = rep["order"] >= 0
        assert g["count"] == rep["count"] == picked.sum(), (label, i)
        assert (rep["q"][picked] >= (1.0 - 1e-9) * rep["best"][picked]).all(), (label, i, rep["q"], rep["best"])
        assert np.array_equal(g["order"], ref["order"]), (label, i, g["order"], ref["order"], ref["margin"])
        assert np.array_equal(g["rank"], rep["rank"]), (label, i)
        err = sr.select_errors(g, rep, n, s0)
        for key, v in err.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(label, worst)
    return worst
