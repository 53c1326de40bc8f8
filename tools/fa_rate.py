"""Rates of the factor-analysis sparse CVI step (vidp_amd.factor_analysis_variational.FactorAnalysisSparseCVI; kernels
mfgm_fa_predict_lik, mfgm_fa_site_update[_q]; csrc/mfgm_fa.h) on one GPU, in one process, the routes interleaved:

    L4D8      four Matern32 latents                 D = 8,  dense sites
    L8D16     eight Matern32 latents                D = 16, packed sites

at M = 20 000 inducing states 0.25 lengthscales apart, N = 200 000 time points and P = 32 Poisson outputs with time-invariant weights.
Per shape one JSON line:

    step_ms       medians of --reps repetitions of `update_sites; classic_elbo` after 3 warm-ups, device synchronisation around each
                  timed window, one repetition of every route in turn:  native (the kernels), torch (the same class under
                  VIDP_NATIVE_FA=0) and materialised: the scalar SparseCVIGaussianProcess step (mfgm_sparse_predict[_kl] +
                  mfgm_sparse_site_update[_q]) on the N P rows w_ip [2D] -- the only route to this model without the kernels
    peak_mb       torch's peak allocated memory over one warm-up step of the route
    bytes         algorithmic bytes of the two kernels: predict-lik N (2D + L + P + 4P + 2L + 2LT) 8 [h, c, y in; fmu, fvar, dm, dv, lmu,
                  gam1, lcov, gam2 out] + (M + 1) (3 D^2 + 2D + 1) 8 [pair marginal blocks, pair mean, ve_part] + P L 8; site update
                  N (2D + L + LT) 8 + 2 (M + 1) (QS + 2D) 8, QS = D (D + 1) + D^2 packed or 4 D^2 dense.  Kernel times come from a
                  profiler run of their own (--native-only keeps everything else out of it): bytes / time is the achieved rate.
    elbo          of every route after the timed steps (they ran the same number of steps)

    usage: python tools/fa_rate.py [--reps 30] [--shapes L4D8,L8D16] [--M 20000] [--N 200000] [--P 32] [--native-only]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DZ = 0.25


def kids(name):
    from vidp_amd import kernels as K
    L = 4 if name == "L4D8" else 8
    return [K.Matern32(0.6 + 0.05 * l, 1.0 - 0.05 * l) for l in range(L)]


def make_data(L, M, N, P):
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(0.0, DZ * M, size=N))
    A = rng.normal(size=(P, L)) * (0.6 / np.sqrt(L))
    g = np.stack([np.sin((0.3 + 0.1 * l) * t + l) for l in range(L)], 1)
    Y = rng.poisson(np.exp(g @ A.T)).astype(np.float64)
    Y[rng.uniform(size=Y.shape) < 0.05] = np.nan
    return t, A, Y


def build(name, z, A, P):
    from vidp_amd import kernels as K
    from vidp_amd.factor_analysis_variational import FactorAnalysisSparseCVI
    from vidp_amd.likelihoods import Poisson
    return FactorAnalysisSparseCVI(K.FactorAnalysisKernel(torch.from_numpy(A), kids(name), P), z, Poisson(1.0), learning_rate=0.5)


def build_materialised(name, z, fa, t, Y):
    """The scalar sparse CVI model on the N P rows: its per-data-set constants (rows, conditional variances, CSR offsets scaled by P) are
    put where SparseCVIGaussianProcess._data keeps them.  NaN observations cannot be given to the scalar model: they are dropped."""
    from vidp_amd import _lib
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.stamps import Stamp
    P = Y.shape[1]
    Hl, c, idx = fa._features(t)
    W = fa._weights(t)
    seen = ~torch.isnan(Y)
    w = torch.einsum("pl,nlj->npj", W, Hl)[seen].contiguous()                     # [rows, 2D]
    cc = torch.einsum("pl,nl->np", W * W, c)[seen].contiguous()
    rows_t = t[:, None].expand(-1, P)[seen].contiguous()
    y = Y[seen][:, None].contiguous()
    M, d = int(z.shape[0]), fa.kernel.state_dim
    seg = torch.zeros(M + 2, dtype=torch.int32, device=z.device)
    seg[1:] = torch.cumsum(torch.bincount(idx[:, None].expand(-1, P)[seen], minlength=M + 1), 0).to(torch.int32)
    m = SparseCVIGaussianProcess(K.IndependentMultiOutput(kids(name)), z, Poisson(1.0), learning_rate=0.5)
    pm = m.kernel.initial_mean(()).to(z.device, torch.float64).contiguous()
    pc = m.kernel.initial_covariance_matrix().to(z.device, torch.float64).contiguous()
    sd = _lib.SparseData()
    sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = M, d, int(w.shape[0]), 0, M + 1
    sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = seg.data_ptr(), w.data_ptr(), cc.data_ptr(), pm.data_ptr(), pc.data_ptr()
    m._data_cache = (Stamp(rows_t), dict(struct=sd, keep=(seg, w, cc, pm, pc), N=int(w.shape[0]), own=slice(None)))
    return m, (rows_t, y)


class Route:
    """A step function and the environment it runs under (the torch route is chosen when a data set's constants are first built)."""

    def __init__(self, step, env=None):
        self.step, self.env, self.ms, self.peak = step, env or {}, [], 0.0

    def run(self, timed):
        os.environ.update(self.env)
        try:
            if not timed:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                out = self.step()
                torch.cuda.synchronize()
                self.peak = torch.cuda.max_memory_allocated() / 2 ** 20
                return out
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = self.step()
            b.record()
            torch.cuda.synchronize()
            self.ms.append(a.elapsed_time(b))
            return out
        finally:
            for k in self.env:
                os.environ.pop(k, None)


def shape(name, M, N, P, reps, native_only):
    z = DZ * torch.arange(M, dtype=torch.float64, device="cuda")
    L = len(kids(name))
    t, A, Y = make_data(L, M, N, P)
    data = (torch.from_numpy(t).cuda(), torch.from_numpy(Y).cuda())
    models = dict(native=build(name, z, A, P))
    step = lambda m, d: (lambda: (m.update_sites(d), m.classic_elbo(d))[1])
    routes = dict(native=Route(step(models["native"], data)))
    if not native_only:
        models["torch"] = build(name, z, A, P)
        routes["torch"] = Route(step(models["torch"], data), {"VIDP_NATIVE_FA": "0"})
        models["materialised"], mdata = build_materialised(name, z, models["native"], *data)
        routes["materialised"] = Route(step(models["materialised"], mdata))
    for _ in range(3):
        for r in routes.values():
            r.run(False)
    elbo = {}
    for _ in range(reps):
        for k, r in routes.items():
            elbo[k] = r.run(True)
    m = models["native"]
    assert m._data(data) is not None and ("torch" not in models or models["torch"]._data(data) is None)
    D, LT = sum(m._dl), L * (L + 1) // 2
    QS = D * (D + 1) + D * D if m._packed else 4 * D * D
    out = dict(shape=name, D=D, L=L, P=P, M=M, N=N, lr=0.5, packed_sites=bool(m._packed), reps=reps,
               step_ms={k: round(float(np.median(r.ms)), 4) for k, r in routes.items()},
               step_ms_min_max={k: [round(min(r.ms), 4), round(max(r.ms), 4)] for k, r in routes.items()},
               peak_mb={k: round(r.peak, 1) for k, r in routes.items()},
               bytes=dict(predict_lik=8 * (N * (2 * D + L + 5 * P + 2 * L + 2 * LT) + (M + 1) * (3 * D * D + 2 * D + 1) + P * L),
                          site_update=8 * (N * (2 * D + L + LT) + 2 * (M + 1) * (QS + 2 * D))),
               elbo={k: float(v) for k, v in elbo.items()})
    m.dist_p.plan.check_info()
    print(json.dumps(out), flush=True)
    del models, routes, data
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="L4D8,L8D16")
    ap.add_argument("--M", type=int, default=20_000)
    ap.add_argument("--N", type=int, default=200_000)
    ap.add_argument("--P", type=int, default=32)
    ap.add_argument("--native-only", action="store_true")
    args = ap.parse_args()
    import vidp_amd  # noqa: F401
    for name in args.shapes.split(","):
        shape(name, args.M, args.N, args.P, args.reps, args.native_only)


if __name__ == "__main__":
    main()
