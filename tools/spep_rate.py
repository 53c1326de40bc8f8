"""Rates of the sparse Power EP site update (mfgm_sparse_pep_sites[_q], csrc/mfgm_spep.h) and of the step that uses it, native route
against the torch route of the same class (VIDP_FUSED_SPARSE=0) on the same machine in the same run:

    c5   config 5's shape: Sum of 4 x Matern-5/2 + 2 x Matern-3/2 (d = 16), 200 000 inducing states 0.1 apart, 400 000 observations
    d3   Matern-5/2 (d = 3), 200 000 inducing states 0.2 lengthscales apart, 400 000 observations

each with Bernoulli and Gaussian observations, alpha = 0.9, lr = 0.5.  Per case one JSON line: `energy_call_ms`, the device-event time
around compute_log_norm() on the native route (the kernel in energy mode, which reads everything the update reads and writes e only,
plus the host glue of the call: an allocation, cache look-ups, the launch), `update_sites()` and `update_sites(); energy()` on both
routes.  Device-event timing, median of --reps runs after a warm-up; the two routes are timed one after the other, native first.

The time of the kernel alone comes from a profiler run of its own,
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/spep_rate.py --kernel-only
which only launches the kernel (3 updates, then --reps energy-mode launches per case; k_spep_sites<KIND, NP> names the case:
KIND 1 Bernoulli, 3 Gaussian; NP 32 for d = 16, 8 for d = 3).

Algorithmic bytes of the kernel per launch: the marginal blocks (M (2 d^2 + d)), the sites read (update: and written back)
((M + 1) (QS + 2d), QS = d (d + 1) + d^2 packed or 4 d^2 dense), w, c, y (N (2d + 2)), seg, e / lnorm -- doubles.

    usage: python tools/spep_rate.py [--reps 10] [--cases c5,d3] [--M 200000]
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
    return sorted(times)[len(times) // 2]


def case(name, M, lik_name, reps, kernel_only=False):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Gaussian, PEPGaussian, PEPScalarLikelihood
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    rng = np.random.default_rng(5)
    if name == "c5":
        ls = np.exp(np.linspace(np.log(0.05), np.log(2.0), 6))
        kern = lambda: K.Sum([K.Matern52(float(l), 1.0) for l in ls[:4]] + [K.Matern32(float(l), 1.0) for l in ls[4:]])
        dz = 0.1
    else:
        kern = lambda: K.Matern52(1.0, 1.0)
        dz = 0.2
    d = kern().state_dim
    z = torch.linspace(0.0, dz * M, M, dtype=torch.float64, device="cuda")
    t = torch.from_numpy(np.sort(rng.uniform(0.0, dz * M, size=2 * M))).cuda()
    f = torch.sin(3.0 * t) + 0.3 * torch.from_numpy(rng.normal(size=2 * M)).cuda()
    if lik_name == "bernoulli":
        y, lik = (f > 0).to(torch.float64)[:, None].contiguous(), lambda: PEPScalarLikelihood(Bernoulli())
    else:
        y, lik = f[:, None].contiguous(), lambda: PEPGaussian(Gaussian(0.09))
    data = (t, y)
    out = dict(case=name, lik=lik_name, d=d, M=M, N=2 * M, alpha=0.9, lr=0.5)
    if kernel_only:
        m = SparsePowerExpectationPropagation(kern(), z, lik(), learning_rate=0.5, alpha=0.9)
        for _ in range(3):
            m.update_sites(data)
        assert m._native(m._data(data))
        for _ in range(reps):
            m.compute_log_norm(data)
        torch.cuda.synchronize()
        return
    for route in ("native", "torch"):
        if route == "torch":
            os.environ["VIDP_FUSED_SPARSE"] = "0"
        try:
            m = SparsePowerExpectationPropagation(kern(), z, lik(), learning_rate=0.5, alpha=0.9)
            for _ in range(3):
                m.update_sites(data)
            if route == "native":
                assert m._native(m._data(data))
                m._marginals()
                k_ms = timed(lambda: m.compute_log_norm(data), reps)
                qs = d * (d + 1) + d * d if m._packed else 4 * d * d
                nbytes = 8 * (M * (2 * d * d + d) + (M + 1) * (qs + 2 * d + 2) + 2 * M * (2 * d + 2))
                out.update(energy_call_ms=round(k_ms, 4), packed=bool(m._packed), algorithmic_bytes=nbytes,
                           share_of_hbm_peak_of_call=round(nbytes / HBM_PEAK / (k_ms * 1e-3), 4))

            def both():
                m.update_sites(data)
                return m.energy(data)
            out[route + "_update_ms"] = round(timed(lambda: m.update_sites(data), reps), 4)
            out[route + "_update_energy_ms"] = round(timed(both, reps), 4)
            out[route + "_energy"] = float(m.energy(data))
            out[route + "_skipped"] = m.num_skipped
            del m
            torch.cuda.empty_cache()
        finally:
            os.environ.pop("VIDP_FUSED_SPARSE", None)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="c5,d3")
    ap.add_argument("--M", type=int, default=200_000)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import vidp_amd  # noqa: F401
    for name in args.cases.split(","):
        for lik_name in ("bernoulli", "gaussian"):
            case(name, args.M, lik_name, args.reps, args.kernel_only)


if __name__ == "__main__":
    main()
