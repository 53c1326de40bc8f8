"""Rates of the posterior sampler (Plan.sample, csrc/mfgm_sample.h) against the natural-layout route (sampling.fallback_sample) on the
posterior of a double-well CVI-DP model after one site update:

    h1   headline posterior, B = 64, T = 100 000, d = 6, S = 1
    h16  headline posterior, S = 16
    c2   one chain, T = 100 000, d = 3, S = 64

Device-event timing, median of --reps runs after a warm-up; one JSON line per shape and route.  Algorithmic bytes: two reads of the factor
(L and G: d (d + 1) / 2 + d^2 doubles per node, 21 + 36 at d = 6) plus the S B T d doubles written.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/sample_rate.py` run.

    usage: python tools/sample_rate.py [--configs h1,h16,c2] [--reps 5] [--no-fallback]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s (MI355X spec)
SHAPES = {"h1": (64, 100_000, 6, 1), "h16": (64, 100_000, 6, 16), "c2": (1, 100_000, 3, 64)}


def posterior(B, T, d):
    import vidp_amd as amd
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    rng = np.random.default_rng(0)
    grid = np.arange(T) * 0.01
    idx = np.arange(10, T - 1, 50)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.2 * rng.normal(size=(B, len(idx), d))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(0.3 * np.eye(d))),
                    prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)), plan=amd.Plan(B, T, d))
    m.update_data_sites(0.5)
    m.update_girsanov_sites(0.2)
    return m.dist_q


def timed(run, reps):
    x = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all())
    del x
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="h1,h16,c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-fallback", action="store_true")
    args = ap.parse_args()
    from vidp_amd import sampling
    for key in args.configs.split(","):
        B, T, d, S = SHAPES[key]
        q = posterior(B, T, d)
        pl, f = q.plan, q._posterior_packed()["f"]
        factor_bytes = B * T * (d * (d + 1) // 2 + d * d) * 8
        nbytes = 2 * factor_bytes + S * B * T * d * 8
        routes = [("native", sampling.native_sample)] + ([] if args.no_fallback else [("fallback", sampling.fallback_sample)])
        for name, fn in routes:
            ms, all_ms = timed(lambda: fn(pl, f, S, 1, 1), args.reps)
            print(json.dumps(dict(shape=key, route=name, B=B, T=T, d=d, S=S, R0=pl.R, P=pl.P, ms=round(ms, 4),
                                  ms_all=[round(x, 4) for x in all_ms], algorithmic_bytes=nbytes,
                                  hbm_bound_ms=round(nbytes / HBM_PEAK * 1e3, 4), share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 4),
                                  packed_out=os.environ.get("MFGM_SAMPLE_PACKED", "0"))), flush=True)
        del q, pl, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
