"""Rates of the panel sparse CVI step (vidp_amd.panel_variational_cvi.PanelSparseCVI; kernels mfgm_panel_theta, mfgm_panel_predict_lik,
mfgm_panel_site_update; csrc/mfgm_panel.h) on one GPU, in one process, the routes interleaved:

    matern52-poisson    Matern-5/2 (d = 3), Poisson
    sum5-bernoulli      Sum([Matern32, Matern52]) (d = 5), Bernoulli

at B = 4096 series, M = 128 inducing states 0.25 lengthscales apart and N = 512 points per series, a tenth of them absent.  Per shape
one JSON line:

    step_ms       medians of --reps repetitions of `update_sites; classic_elbo` after 3 warm-ups, device synchronisation around each
                  timed window, one repetition of every route in turn:  native (the kernels), torch (the same class under
                  VIDP_NATIVE_PANEL=0) and loop32: --loop single-chain SparseCVIGaussianProcess models, one per series over the first
                  32 series with their present points, stepped back to back
    loop_extrapolated_ms   loop32 scaled by B / 32: AN EXTRAPOLATION, not a measurement (nobody steps 4096 Python models here)
    bytes         algorithmic bytes of the three kernels.  theta: B (M + 1) (3 d^2 + 2d) 8 [the three site quadrants and nat1 in]
                  + B M (d + d (d + 1) / 2 + d^2) 8 [packed lin, diag, sub out]; predict-lik: B N (2d + 7) 8 - B N 4 [w, c, y, idx (int32)
                  in; fmu, fvar, g1, g2 out] + B M (d + d (d + 1) / 2 + d^2) 8 [packed marginals] + B 8; site update: B N (2d + 2) 8
                  + B (M + 2) 4 + 2 B (M + 1) (4 d^2 + 2d) 8.  Kernel times come from a profiler run of their own (--native-only keeps
                  everything else out of it): bytes / time is the achieved rate, to be set against the HBM peak.
    elbo          of every route after the timed steps (they ran the same number of steps; loop32 covers 32 series only)

Run every shape as a command of its own under a time limit, so that trouble ends it:

    timeout -k 10 600 python tools/panel_rate.py --shapes matern52-poisson
    timeout -k 10 600 python tools/panel_rate.py --shapes sum5-bernoulli
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/panel_rate.py --native-only --reps 10 --shapes ...

    usage: python tools/panel_rate.py [--reps 30] [--shapes matern52-poisson,sum5-bernoulli] [--B 4096] [--M 128] [--N 512] [--loop 32]
                                      [--native-only]
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


def kernel(name):
    from vidp_amd import kernels as K
    if name == "matern52-poisson":
        return K.Matern52(1.0, 0.8)
    return K.Sum([K.Matern32(0.8, 0.6), K.Matern52(1.0, 0.4)])


def likelihood(name):
    from vidp_amd.likelihoods import Bernoulli, Poisson
    return Poisson(1.3) if name == "matern52-poisson" else Bernoulli(1e-3)


def make_data(name, B, M, N):
    from scipy import special
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(0.0, DZ * M, size=(B, N)), axis=1)
    f = 0.8 * np.sin(0.9 * t + rng.uniform(0, 6, size=(B, 1)))
    if name == "matern52-poisson":
        y = rng.poisson(np.exp(f + 0.2)).astype(np.float64)
    else:
        y = (rng.uniform(size=t.shape) < 0.5 * special.erfc(-f / np.sqrt(2.0))).astype(np.float64)
    y[rng.uniform(size=t.shape) < 0.1] = np.nan
    return t, y


class Route:
    """A step function and the environment it runs under."""

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


def shape(name, B, M, N, reps, loop, native_only):
    from vidp_amd.panel_variational_cvi import PanelSparseCVI
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    z = DZ * torch.arange(M, dtype=torch.float64, device="cuda")
    t, y = make_data(name, B, M, N)
    data = (torch.from_numpy(t).cuda(), torch.from_numpy(y[..., None]).cuda())
    new = lambda: PanelSparseCVI(kernel(name), z, likelihood(name), B, learning_rate=0.5)
    models = dict(native=new())
    step = lambda m: (lambda: (m.update_sites(data), m.classic_elbo(data))[1])
    routes = dict(native=Route(step(models["native"])))
    assert models["native"]._native()
    if not native_only:
        models["torch"] = new()
        routes["torch"] = Route(step(models["torch"]), {"VIDP_NATIVE_PANEL": "0"})
        loop = min(loop, B)
        parts = [SparseCVIGaussianProcess(kernel(name), z, likelihood(name), learning_rate=0.5) for _ in range(loop)]
        pdata = []
        for b in range(loop):
            ok = ~np.isnan(y[b])
            pdata.append((torch.from_numpy(t[b][ok]).cuda(), torch.from_numpy(y[b][ok][:, None]).cuda()))

        def looped():
            tot = 0.0
            for p, pd in zip(parts, pdata):
                p.update_sites(pd)
                tot = tot + p.classic_elbo(pd)
            return tot
        routes[f"loop{loop}"] = Route(looped)
    for _ in range(3):
        for r in routes.values():
            r.run(False)
    elbo = {}
    for _ in range(reps):
        for k, r in routes.items():
            elbo[k] = r.run(True)
    d = models["native"].kernel.state_dim
    node = d + d * (d + 1) // 2 + d * d
    med = {k: float(np.median(r.ms)) for k, r in routes.items()}
    out = dict(shape=name, d=d, B=B, M=M, N=N, lr=0.5, reps=reps, step_ms={k: round(v, 4) for k, v in med.items()},
               step_ms_min_max={k: [round(min(r.ms), 4), round(max(r.ms), 4)] for k, r in routes.items()},
               bytes=dict(theta=8 * (B * (M + 1) * (3 * d * d + 2 * d) + B * M * node),
                          predict_lik=8 * (B * N * (2 * d + 7) + B * M * node + B) - 4 * B * N,
                          site_update=8 * (B * N * (2 * d + 2) + 2 * B * (M + 1) * (4 * d * d + 2 * d)) + 4 * B * (M + 2)),
               elbo={k: float(v) for k, v in elbo.items()})
    if not native_only:
        out["loop_extrapolated_ms"] = dict(value=round(med[f"loop{loop}"] * B / loop, 2), note=f"loop{loop} x B / {loop}: an extrapolation")
    models["native"].dist_p.plan.check_info()
    print(json.dumps(out), flush=True)
    del models, routes, data
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="matern52-poisson,sum5-bernoulli")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--M", type=int, default=128)
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--native-only", action="store_true")
    args = ap.parse_args()
    import vidp_amd  # noqa: F401
    for name in args.shapes.split(","):
        shape(name, args.B, args.M, args.N, args.reps, args.loop, args.native_only)


if __name__ == "__main__":
    main()
