"""Rates of the linear-readout likelihood of the diffusion models (likelihoods.LinearReadout; kernels mfgm_readout_site_update /
mfgm_readout_obs_ve, csrc/mfgm_readout.h) at the headline shape on the dense route: CVISitesSDE, double well, B = 64, T = 100 000,
d = 6, 1 000 observations per trajectory (every 100th node), data from a seed.

    models   gauss2   o = 2 Gaussian rows
             mixed3   o = 3, one Gaussian, one Poisson and one Bernoulli row
    timed    sites    update_data_sites(0.5), after an untimed classic_elbo() (the state the loop reaches it in: refreshed marginals)
             step     update_data_sites(0.5); update_girsanov_sites(0.2); classic_elbo()
    routes   native   one launch each for the site update and the variational expectations
             torch    the same object with native_readout off (VIDP_NATIVE_READOUT=0): gather, projections, the scalar-likelihood
                      kernel, back-projections, blend and scatter as separate launches

The two routes alternate inside every repetition (same object, same state sequence); device-event timing, medians of --reps
repetitions after a warm-up; one JSON line per (model, quantity).  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/readout_rate.py --reps 5` run.

    usage: python tools/readout_rate.py [--reps 30] [--B 64] [--T 100000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def model(name, B, T, d=6, every=100):
    from vidp_amd import likelihoods as L, sde as gsde
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    rng = np.random.default_rng(71892305 + len(name))
    grid = np.arange(T) * 0.01
    idx = np.arange(every // 2, T, every)
    n = len(idx)
    if name == "gauss2":
        H = rng.normal(size=(2, d)) / np.sqrt(d)
        lik = L.LinearReadout(H, L.Gaussian(0.09))
        y = rng.normal(size=(B, n, 2))
    else:
        H = rng.normal(size=(3, d)) / np.sqrt(d)
        lik = L.LinearReadout(H, [L.Gaussian(0.09), L.Poisson(1.0), L.Bernoulli()], offset=[0.0, 0.5, 0.0])
        y = np.stack([rng.normal(size=(B, n)), rng.poisson(2.0, size=(B, n)), rng.integers(0, 2, size=(B, n))], -1).astype(np.float64)
    m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], torch.from_numpy(y).cuda()), lik,
                    prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)))
    return m, n


def timed(run, prep=None):
    if prep is not None:
        prep()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--models", default="gauss2,mixed3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this path"
    for name in args.models.split(","):
        m, n = model(name, args.B, args.T)

        def sites():
            m.update_data_sites(0.5)

        def step():
            m.update_data_sites(0.5)
            m.update_girsanov_sites(0.2)
            return m.classic_elbo()

        for quantity, run, prep in (("sites", sites, m.classic_elbo), ("step", step, None)):
            ms = dict(native=[], torch=[])
            for rep in range(args.reps + 2):
                for route in ("native", "torch"):
                    m.native_readout = route == "native"
                    assert (m._readout_native() is not None) == (route == "native") and m._cq is None
                    t = timed(run, prep)
                    if rep >= 2:      # two warm-up repetitions per route
                        ms[route].append(t)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            emit(model=name, quantity=quantity, B=args.B, T=args.T, d=6, n_obs=n, reps=args.reps, ms_native=round(med["native"], 4),
                 ms_torch=round(med["torch"], 4), native_over_torch=round(med["native"] / med["torch"], 4),
                 ms_native_minmax=[round(min(ms["native"]), 4), round(max(ms["native"]), 4)],
                 ms_torch_minmax=[round(min(ms["torch"]), 4), round(max(ms["torch"]), 4)], elbo=float(m.classic_elbo()))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
