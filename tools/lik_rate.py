"""Rates of the scalar non-Gaussian likelihoods (mfgm_scalar_lik, csrc/mfgm_lik.h) and of the CVI-GP step that uses them:

    kernel   mfgm_scalar_lik alone (VE, g1, g2 written), n = 1e5 and 1e6, Bernoulli-probit and Poisson-exp
    step     config 2's model (Matern-5/2, T = 100 000, one chain; bench.py c2) with y = 1[sin(12 t) + 0.1 noise > 0] from a seed:
             `update_sites(); elbo()` with Bernoulli() eagerly and through step_graph(), and with the same log density through
             ScalarQuadratureLikelihood (the torch route); the Gaussian config-2 step on the same device as the yardstick

Device-event timing, median of --reps runs after a warm-up; one JSON line per case.  Algorithmic bytes of the kernel: three [n] reads and
three [n] writes.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/lik_rate.py` run.

    usage: python tools/lik_rate.py [--reps 20] [--cases kernel,step]
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


def timed(run, reps):
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], times


def emit(**kw):
    print(json.dumps(kw), flush=True)


def kernel_cases(reps):
    import vidp_amd
    from vidp_amd.packed import _ptr, _stream
    lib = vidp_amd._lib.load()
    rng = np.random.default_rng(0)
    for n in (100_000, 1_000_000):
        mu = torch.from_numpy(rng.uniform(-3, 3, size=n)).cuda()
        var = torch.from_numpy(10.0 ** rng.uniform(-3, 0, size=n)).cuda()
        for kind, name, param in ((1, "bernoulli", 1e-3), (2, "poisson", 1.0)):
            y = torch.from_numpy((rng.uniform(size=n) < 0.5).astype(np.float64) if kind == 1 else rng.poisson(2.0, size=n).astype(np.float64)).cuda()
            out = [torch.empty_like(mu) for _ in range(3)]

            def run():
                vidp_amd._lib.check(lib.mfgm_scalar_lik(kind, n, _ptr(mu), _ptr(var), _ptr(y), param, *(_ptr(o) for o in out), _stream()),
                                    "mfgm_scalar_lik")
            ms, all_ms = timed(run, reps)
            nbytes = 6 * n * 8
            emit(case="kernel", lik=name, n=n, ms=round(ms, 5), ms_all=[round(x, 5) for x in all_ms], algorithmic_bytes=nbytes,
                 share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 4), ns_per_obs=round(ms * 1e6 / n, 4))


def c2_model(lik, binary):
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import CVIGaussianProcess
    T = 100_000
    rng = np.random.default_rng(71892305 + 2)
    t = torch.linspace(0, 0.01 * T, T, dtype=torch.float64, device="cuda")
    f = torch.sin(12 * t) + 0.1 * torch.from_numpy(rng.normal(size=T)).cuda()
    y = ((f > 0).to(torch.float64) if binary else f)[:, None].contiguous()
    return CVIGaussianProcess((t, y), K.Matern52(lengthscale=0.2, variance=1.0), lik, learning_rate=0.5)


def step_cases(reps):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, ScalarQuadratureLikelihood
    for name, mk, binary in (("gaussian", lambda: Gaussian(0.01), False), ("bernoulli", Bernoulli, True),
                             ("bernoulli_torch_route", lambda: ScalarQuadratureLikelihood(Bernoulli()._log_prob), True)):
        m = c2_model(mk(), binary)

        def eager():
            m.update_sites()
            return m.elbo()
        ms, all_ms = timed(eager, reps)
        e = float(eager())
        emit(case="step", lik=name, route="eager", T=100_000, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms], elbo=e)
        if name != "bernoulli_torch_route":
            step = m.step_graph()
            ms, all_ms = timed(step, reps)
            emit(case="step", lik=name, route="graph", T=100_000, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms], elbo=float(step()))
        del m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="kernel,step")
    args = ap.parse_args()
    import vidp_amd  # noqa: F401
    cases = args.cases.split(",")
    if "kernel" in cases:
        kernel_cases(args.reps)
    if "step" in cases:
        step_cases(args.reps)


if __name__ == "__main__":
    main()
