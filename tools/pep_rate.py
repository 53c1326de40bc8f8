"""Rates of the Power Expectation Propagation site update (mfgm_pep_sites, csrc/mfgm_pep.h) and of the PEP step that uses it:

    kernel   mfgm_pep_sites alone over all points (sites and log normalisers updated in place, lr = 0.5), n = 1e5 and 1e6, Gaussian,
             Bernoulli-probit and Poisson-exp, alpha = 1 and 0.9 (Bernoulli at alpha = 1 takes the closed form, the rest the rule)
    step     config 2's model (Matern-5/2, T = 100 000, one chain; bench.py c2) with y = 1[sin(12 t) + 0.1 noise > 0] from a seed and
             PEPScalarLikelihood(Bernoulli()), alpha = 0.9, lr = 0.5: `update_sites(); elbo()` eagerly and through step_graph(), and
             `update_sites(); energy()`; CVIGaussianProcess(Bernoulli()) `update_sites(); elbo()` on the same data as the yardstick

Device-event timing, median of --reps runs after a warm-up; one JSON line per case.  Algorithmic bytes of the kernel: five [n] reads
(mu, v, y, eta1, eta2) and three [n] read-writes (eta1, eta2, l) -- 8 n doubles, counting the log normaliser's read once.

    usage: python tools/pep_rate.py [--reps 20] [--cases kernel,step]
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
        for kind, name, param in ((3, "gaussian", 0.5), (1, "bernoulli", 1e-3), (2, "poisson", 1.0)):
            if kind == 1:
                yh = (rng.uniform(size=n) < 0.5).astype(np.float64)
            elif kind == 2:
                yh = rng.poisson(2.0, size=n).astype(np.float64)
            else:
                yh = rng.normal(size=n)
            y = torch.from_numpy(yh).cuda()
            for alpha in (1.0, 0.9):
                # sites with proper cavities that stay proper under repeated damped updates: small site precisions
                n1 = torch.zeros(n, dtype=torch.float64, device="cuda")
                n2 = torch.full((n,), -1e-3, dtype=torch.float64, device="cuda")
                ln = torch.zeros(n, dtype=torch.float64, device="cuda")
                sk = torch.zeros(1, dtype=torch.int32, device="cuda")

                def run():
                    n1.zero_()
                    n2.fill_(-1e-3)
                    vidp_amd._lib.check(lib.mfgm_pep_sites(kind, n, _ptr(mu), _ptr(var), _ptr(y), param, alpha, 0.5, None, 0, _ptr(n1),
                                                           _ptr(n2), _ptr(ln), None, _ptr(sk), _stream()), "mfgm_pep_sites")

                def reset_only():
                    n1.zero_()
                    n2.fill_(-1e-3)
                ms, all_ms = timed(run, reps)
                ms0, _ = timed(reset_only, reps)
                k_ms = max(ms - ms0, 1e-6)
                nbytes = 8 * n * 8
                emit(case="kernel", lik=name, alpha=alpha, n=n, ms=round(k_ms, 5), ms_with_reset=round(ms, 5), reset_ms=round(ms0, 5),
                     ms_all=[round(x, 5) for x in all_ms], algorithmic_bytes=nbytes,
                     share_of_hbm_bound=round(nbytes / HBM_PEAK / (k_ms * 1e-3), 4), ns_per_point=round(k_ms * 1e6 / n, 4),
                     skipped=int(sk.item()))


def c2_data():
    T = 100_000
    rng = np.random.default_rng(71892305 + 2)
    t = torch.linspace(0, 0.01 * T, T, dtype=torch.float64, device="cuda")
    f = torch.sin(12 * t) + 0.1 * torch.from_numpy(rng.normal(size=T)).cuda()
    return t, (f > 0).to(torch.float64)[:, None].contiguous()


def step_cases(reps):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, PEPScalarLikelihood
    from vidp_amd.pep import PowerExpectationPropagation
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t, y = c2_data()
    kern = lambda: K.Matern52(lengthscale=0.2, variance=1.0)
    m = PowerExpectationPropagation((t, y), kern(), PEPScalarLikelihood(Bernoulli()), learning_rate=0.5, alpha=0.9)

    def eager():
        m.update_sites()
        return m.elbo()

    def with_energy():
        m.update_sites()
        return m.energy()
    ms, all_ms = timed(eager, reps)
    emit(case="step", model="pep", step="update_sites+elbo", route="eager", T=100_000, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms],
         elbo=float(eager()))
    ms, all_ms = timed(with_energy, reps)
    emit(case="step", model="pep", step="update_sites+energy", route="eager", T=100_000, ms=round(ms, 4),
         ms_all=[round(x, 4) for x in all_ms], energy=float(with_energy()))
    step = m.step_graph()
    ms, all_ms = timed(step, reps)
    emit(case="step", model="pep", step="update_sites+elbo", route="graph", T=100_000, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms],
         elbo=float(step()), skipped=m.num_skipped)
    del m, step
    torch.cuda.empty_cache()
    c = CVIGaussianProcess((t, y), kern(), Bernoulli(), learning_rate=0.5)

    def cvi():
        c.update_sites()
        return c.elbo()
    ms, all_ms = timed(cvi, reps)
    emit(case="step", model="cvi", step="update_sites+elbo", route="eager", T=100_000, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms],
         elbo=float(cvi()))
    step = c.step_graph()
    ms, all_ms = timed(step, reps)
    emit(case="step", model="cvi", step="update_sites+elbo", route="graph", T=100_000, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms],
         elbo=float(step()))


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
