"""Rates of the spatio-temporal sparse CVI step (vidp_amd.spatio_temporal_variational.SpatioTemporalSparseCVI) and of its two kernels
(mfgm_st_predict_kl, mfgm_st_site_update_q; csrc/mfgm_st.h) on one GPU, against the same step on the materialised w [N, 2D] through
mfgm_sparse_predict_kl + mfgm_sparse_site_update_q (VIDP_ST_FACTORED=0), in the same process, the two routes interleaved:

    d16   Ms = 8,  Matern-3/2 in time (D = 16), M_t = 20 000 inducing times 0.05 lengthscales apart, N = 2 000 000 points, p = 2
    d30   Ms = 10, Matern-5/2 in time (D = 30), same M_t and N

Per shape one JSON line:
    kernels            each kernel alone on both routes (device events around the library call, median of --reps), its algorithmic
                       bytes and their share of the HBM peak
    step_ms            `update_sites(); classic_elbo()` per route: --rounds rounds, in each --reps steps of the factored route then
                       --reps of the materialised one after 3 warm-ups; the median of every round and the median of those
    spread_ms          max - min of the materialised route's round medians; `not_slower` is factored <= materialised + spread
    peak_bytes         torch.cuda.max_memory_allocated over two steps of each route alone (the data set's constants resident, their
                       construction excluded), and the difference next to N 2D 8

Gaussian observations (the cheapest likelihood glue, so the kernels weigh most).  Algorithmic bytes, doubles: predict
N (Ms + 2 d_t + 3) [a, h, c, fmu, fvar] or N (2D + 3), + M (4 D^2 + 2 D) marginal and prior blocks; site update N (Ms + 2 d_t + 2) or
N (2D + 2), + 2 (M + 1) (QS + 2D) sites read and written, QS = D (D + 1) + D^2.

    usage: python tools/st_rate.py [--reps 20] [--rounds 3] [--shapes d16,d30] [--M 20000] [--N 2000000]
"""
import argparse
import ctypes
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s (MI355X spec)
SHAPES = {"d16": (8, 2), "d30": (10, 3)}


def times(run, reps, warm=3):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def median(x):
    return float(np.median(x))


def build(Ms, order, M, N, factored, data=None):
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    dz = 0.05
    zt = dz * torch.arange(M, dtype=torch.float64, device="cuda")
    g = np.meshgrid(np.linspace(-1.0, 1.0, Ms // 2), [-0.4, 0.4], indexing="ij")
    zs = torch.from_numpy(np.stack([g[0].reshape(-1), g[1].reshape(-1)], axis=1)).cuda()
    if data is None:
        rng = np.random.default_rng(5)
        X = np.concatenate([rng.uniform(-1.2, 1.2, size=(N, 2)), np.sort(rng.uniform(0.0, dz * M, size=N))[:, None]], axis=1)
        y = np.sin(0.8 * X[:, -1]) * np.cos(X[:, 0]) + 0.3 * rng.normal(size=N)
        data = (torch.from_numpy(X).cuda(), torch.from_numpy(y[:, None]).cuda())
    kt = K.Matern32(1.0, 1.0) if order == 2 else K.Matern52(1.0, 1.0)
    os.environ["VIDP_ST_FACTORED"] = "1" if factored else "0"
    try:
        m = SpatioTemporalSparseCVI(zs, zt, SK.Matern32([0.9, 1.2], 1.0), kt, Gaussian(0.09), learning_rate=0.5)
        assert m._data(data)["factored"] == factored and m._packed
    finally:
        os.environ.pop("VIDP_ST_FACTORED", None)
    return m, data


def step(m, data):
    m.update_sites(data)
    return m.classic_elbo(data)


def kernel_times(m, data, reps):
    """Device-event medians of the predict and the site-update call of m's route, on its own marginals and on copies of its sites."""
    from vidp_amd import _lib
    from vidp_amd.packed import _ptr, _stream
    d = m._data(data)
    mg, pn, pl = m._marginals(), m._prior_natural(), m.dist_p.plan
    N = d["N"]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda")
    kt = torch.empty(2, dtype=torch.float64, device="cuda")
    g1, g2 = torch.randn(N, dtype=torch.float64, device="cuda"), -torch.rand(N, dtype=torch.float64, device="cuda")
    n1, n2 = m._nat1.clone(), m._nat2q.clone()
    lib, st = pl.lib, ctypes.byref(d["struct"])
    pred = lib.mfgm_st_predict_kl if d["factored"] else lib.mfgm_sparse_predict_kl
    upd = lib.mfgm_st_site_update_q if d["factored"] else lib.mfgm_sparse_site_update_q
    run_p = lambda: _lib.check(pred(st, _ptr(mg["mu"]), _ptr(mg["Sig"]), _ptr(mg["Sub"]), _ptr(out[0]), _ptr(out[1]), pl.h,
                                    _ptr(pn["nat"]["diag"]), _ptr(pn["nat"]["sub"]), -2.0, -1.0, _ptr(m._prior_mean_packed()), _ptr(kt[0:1]),
                                    _ptr(kt[1:2]), _ptr(pl.ws), _stream()), "predict")
    run_u = lambda: _lib.check(upd(st, _ptr(g1), _ptr(g2), 0.5, _ptr(n1), _ptr(n2), _stream()), "site update")
    return median(times(run_p, reps)), median(times(run_u, reps))


def peak(Ms, order, M, N, factored, data):
    m, _ = build(Ms, order, M, N, factored, data)
    step(m, data)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(2):
        step(m, data)
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated()
    del m
    gc.collect()
    torch.cuda.empty_cache()
    return p


def shape(name, M, N, reps, rounds):
    Ms, order = SHAPES[name]
    d_t = order
    D = Ms * d_t
    data = build(Ms, order, M, N, True)[1]
    gc.collect()
    torch.cuda.empty_cache()
    out = dict(shape=name, Ms=Ms, d_t=d_t, D=D, M_t=M, N=N, p=2, lik="gaussian", lr=0.5)
    out["peak_bytes"] = dict(factored=peak(Ms, order, M, N, True, data), materialised=peak(Ms, order, M, N, False, data))
    out["peak_bytes"]["difference"] = out["peak_bytes"]["materialised"] - out["peak_bytes"]["factored"]
    out["peak_bytes"]["N_2D_8"] = N * 2 * D * 8
    a, _ = build(Ms, order, M, N, True, data)
    b, _ = build(Ms, order, M, N, False, data)
    for m in (a, b):
        for _ in range(3):
            step(m, data)
    QS = D * (D + 1) + D * D
    blocks = 8 * M * (4 * D * D + 2 * D)
    sites = 8 * 2 * (M + 1) * (QS + 2 * D)
    kern = {}
    for route, m, per in (("factored", a, Ms + 2 * d_t), ("materialised", b, 2 * D)):
        tp, tu = kernel_times(m, data, reps)
        bp, bu = 8 * N * (per + 3) + blocks, 8 * N * (per + 2) + sites
        kern[route] = dict(predict_kl_ms=round(tp, 4), predict_kl_bytes=bp, predict_kl_share_of_hbm_peak=round(bp / HBM_PEAK / (tp * 1e-3), 4),
                           site_update_ms=round(tu, 4), site_update_bytes=bu, site_update_share_of_hbm_peak=round(bu / HBM_PEAK / (tu * 1e-3), 4))
    out["kernels"] = kern
    meds = dict(factored=[], materialised=[])
    for _ in range(rounds):
        meds["factored"].append(median(times(lambda: step(a, data), reps)))
        meds["materialised"].append(median(times(lambda: step(b, data), reps)))
    fa, ma = median(meds["factored"]), median(meds["materialised"])
    spread = max(meds["materialised"]) - min(meds["materialised"])
    out["step_ms"] = dict(factored=round(fa, 4), materialised=round(ma, 4), factored_rounds=[round(x, 4) for x in meds["factored"]],
                          materialised_rounds=[round(x, 4) for x in meds["materialised"]])
    out["spread_ms"] = round(spread, 4)
    out["not_slower"] = bool(fa <= ma + spread)
    out["elbo"] = dict(factored=float(a.classic_elbo(data)), materialised=float(b.classic_elbo(data)))
    a.dist_p.plan.check_info()
    print(json.dumps(out), flush=True)
    del a, b, data
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="d16,d30")
    ap.add_argument("--M", type=int, default=20_000)
    ap.add_argument("--N", type=int, default=2_000_000)
    args = ap.parse_args()
    import vidp_amd  # noqa: F401
    for name in args.shapes.split(","):
        shape(name, args.M, args.N, args.reps, args.rounds)


if __name__ == "__main__":
    main()
