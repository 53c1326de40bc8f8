"""Rates of the multi-latent sparse CVI step (vidp_amd.multi_latent_variational.MultiLatentSparseCVI; kernels mfgm_ml_predict_lik,
mfgm_ml_site_update[_q]; csrc/mfgm_ml.h) on one GPU, in one process, the routes interleaved:

    hetgauss16    HeteroskedasticGaussian on two Sum([Matern52, Matern52, Matern32])        D = 16, packed sites
    multistage6   MultiStageLikelihood on three Matern32                                    D = 6,  dense sites
    multistage9   MultiStageLikelihood on three Matern52                                    D = 9,  packed sites

at M = 200 000 inducing states 0.25 lengthscales apart and N = 400 000 observations (config 5's shape).  Per shape one JSON line:

    step_ms       medians of --reps repetitions of `update_sites; classic_elbo` after 3 warm-ups, device synchronisation around each
                  timed window, one repetition of every route in turn:  native (the kernels), torch (the same class under
                  VIDP_NATIVE_ML=0) and, for MultiStage, scalar3: the three scalar native SparseCVIGaussianProcess models of the
                  decomposition (Bernoulli on all points, Bernoulli on y >= 1, Poisson on y >= 2) stepped back to back -- the only way
                  to fit this likelihood without the model
    bytes         algorithmic bytes of the two kernels: predict-lik N (2D + L + 1 + 4L) 8 [h, c, y in; fmu, fvar, g1, g2 out]
                  + (M + 1) (3 sum dl^2 + 2D + 1) 8 [within-latent marginal blocks, pair mean, ve_part]; site update N (2D + 2L) 8
                  + 2 (M + 1) (QS + 2D) 8, QS = D (D + 1) + D^2 packed or 4 D^2 dense.  Kernel times come from a profiler run of
                  their own (--native-only keeps everything else out of it): bytes / time is the achieved rate.
    elbo          of every route after the timed steps (they ran the same number of steps)

    usage: python tools/ml_rate.py [--reps 30] [--shapes hetgauss16,multistage6,multistage9] [--M 200000] [--N 400000] [--native-only]
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
    if name == "hetgauss16":
        return [K.Sum([K.Matern52(1.0, 0.6), K.Matern52(0.7, 0.3), K.Matern32(0.8, 0.1)]),
                K.Sum([K.Matern52(1.0, 0.3), K.Matern52(0.6, 0.1), K.Matern32(0.9, 0.1)])]
    if name == "multistage6":
        return [K.Matern32(1.0, 1.0), K.Matern32(0.8, 0.8), K.Matern32(1.0, 0.25)]
    return [K.Matern52(1.0, 1.0), K.Matern52(0.8, 0.8), K.Matern52(0.9, 0.25)]


def make_data(name, M, N):
    from scipy import special
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(0.0, DZ * M, size=N))
    if name == "hetgauss16":
        y = np.sin(0.8 * t) + np.exp(0.5 * (0.6 * np.cos(0.4 * t) - 1.0)) * rng.normal(size=N)
    else:
        p0 = 0.5 * special.erfc(-(0.8 * np.sin(0.9 * t)) / np.sqrt(2.0))
        p1 = 0.5 * special.erfc(-(0.6 * np.cos(0.5 * t)) / np.sqrt(2.0))
        e0, e1 = rng.uniform(size=N) < p0, rng.uniform(size=N) < p1
        y = np.where(e0, 0.0, np.where(e1, 1.0, 2.0 + rng.poisson(np.exp(0.4 * np.sin(0.3 * t) + 0.2))))
    return t, y


def build(name, z):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import HeteroskedasticGaussian, MultiStageLikelihood
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    lik = HeteroskedasticGaussian() if name == "hetgauss16" else MultiStageLikelihood(1e-3, 1.0)
    return MultiLatentSparseCVI(K.IndependentMultiOutput(kids(name)), z, lik, learning_rate=0.5)


class Route:
    """A step function and the environment it runs under (the torch route is chosen when a data set's constants are first built)."""

    def __init__(self, step, env=None):
        self.step, self.env, self.ms = step, env or {}, []

    def run(self, timed):
        os.environ.update(self.env)
        try:
            if not timed:
                return self.step()
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


def shape(name, M, N, reps, native_only):
    from vidp_amd.likelihoods import Bernoulli, Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    z = DZ * torch.arange(M, dtype=torch.float64, device="cuda")
    t, y = make_data(name, M, N)
    data = (torch.from_numpy(t).cuda(), torch.from_numpy(y[:, None]).cuda())
    models = dict(native=build(name, z))
    routes = dict(native=Route(lambda: (models["native"].update_sites(data), models["native"].classic_elbo(data))[1]))
    if not native_only:
        models["torch"] = build(name, z)
        routes["torch"] = Route(lambda: (models["torch"].update_sites(data), models["torch"].classic_elbo(data))[1], {"VIDP_NATIVE_ML": "0"})
        if name != "hetgauss16":
            sub = [(np.ones(N, bool), (y == 0).astype(np.float64)), (y >= 1, (y == 1).astype(np.float64)), (y >= 2, y - 2.0)]
            parts = [SparseCVIGaussianProcess(k, z, lik, learning_rate=0.5)
                     for k, lik in zip(kids(name), (Bernoulli(1e-3), Bernoulli(1e-3), Poisson(1.0)))]
            pdata = [(torch.from_numpy(t[s]).cuda(), torch.from_numpy(lab[s][:, None]).cuda()) for s, lab in sub]

            def scalar3():
                tot = 0.0
                for p, pd in zip(parts, pdata):
                    p.update_sites(pd)
                    tot = tot + p.classic_elbo(pd)
                return tot
            routes["scalar3"] = Route(scalar3)
    for _ in range(3):
        for r in routes.values():
            r.run(False)
    elbo = {}
    for _ in range(reps):
        for k, r in routes.items():
            elbo[k] = r.run(True)
    m = models["native"]
    assert m._data(data) is not None and ("torch" not in models or models["torch"]._data(data) is None)
    dl = m._dl
    D, L = sum(dl), len(dl)
    QS = D * (D + 1) + D * D if m._packed else 4 * D * D
    out = dict(shape=name, D=D, L=L, dl=dl, M=M, N=N, lr=0.5, packed_sites=bool(m._packed), reps=reps,
               step_ms={k: round(float(np.median(r.ms)), 4) for k, r in routes.items()},
               step_ms_min_max={k: [round(min(r.ms), 4), round(max(r.ms), 4)] for k, r in routes.items()},
               bytes=dict(predict_lik=8 * (N * (2 * D + L + 1 + 4 * L) + (M + 1) * (3 * sum(n * n for n in dl) + 2 * D + 1)),
                          site_update=8 * (N * (2 * D + 2 * L) + 2 * (M + 1) * (QS + 2 * D))),
               elbo={k: float(v) for k, v in elbo.items()})
    m.dist_p.plan.check_info()
    print(json.dumps(out), flush=True)
    del models, routes, data
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="hetgauss16,multistage6,multistage9")
    ap.add_argument("--M", type=int, default=200_000)
    ap.add_argument("--N", type=int, default=400_000)
    ap.add_argument("--native-only", action="store_true")
    args = ap.parse_args()
    import vidp_amd  # noqa: F401
    for name in args.shapes.split(","):
        shape(name, args.M, args.N, args.reps, args.native_only)


if __name__ == "__main__":
    main()
