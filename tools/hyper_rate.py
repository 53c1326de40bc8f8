"""Rates of the hyper-parameter score: the entry point mfgm_packed_kernel_score (csrc/mfgm_score.h) alone
(variant "kernel": an event time over its memset and two launches -- launch latency on one chain, not a kernel time),
log_likelihood_and_grad() against log_likelihood() alone, and -- case (a) only -- the one earlier route to the same gradient,
classic_elbo_tape_hyper forward plus backward at the Gaussian-optimal sites.  T = 100 000:

    a   config 2's chain (bench.py c2): Matern-5/2 (d = 3), one chain, CVIGaussianProcess with a Gaussian likelihood after one
        update_sites() at learning rate 1
    b   Sum(Matern52, Matern52, Matern32) (d = 8), B = 64, GaussianProcessRegression

Device-event timing; the variants of a case are INTERLEAVED (one run of each per repetition, in one process) and the median of --reps
repetitions is reported, one JSON line per variant.  The score kernel's algorithmic bytes are (d + d (d + 1) / 2 + d^2) 8 per node plus
the gaps, reported as a share of the 8 TB/s peak.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/hyper_rate.py --cases kernel` run.

    usage: python tools/hyper_rate.py [--reps 30] [--cases kernel,model,tape] [--only a|b]
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
T = 100_000


def interleaved(runs, reps):
    """{name: (median ms, all ms)} of the callables in `runs`, one run of each per repetition after a warm-up of each."""
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(reps):
        for n, run in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            times[n].append(a.elapsed_time(b))
    return {n: (sorted(v)[len(v) // 2], v) for n, v in times.items()}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def case_a():
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    rng = np.random.default_rng(71892305 + 2)
    t = torch.linspace(0, 0.01 * T, T, dtype=torch.float64, device="cuda")
    y = (torch.sin(12 * t) + 0.1 * torch.from_numpy(rng.normal(size=T)).cuda())[:, None].contiguous()
    k = K.Matern52(lengthscale=0.2, variance=1.0)
    m = CVIGaussianProcess((t, y), k, Gaussian(0.01), learning_rate=1.0)
    m.update_sites()
    return "a", "Matern52 (config 2), B = 1", k, m, t[None], 1


def case_b():
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    rng = np.random.default_rng(3)
    B = 64
    t = torch.from_numpy(np.cumsum(0.01 * (1.0 + 0.1 * rng.uniform(-1, 1, size=(B, T))), axis=-1)).cuda()
    y = (torch.sin(12 * t) + 0.1 * torch.from_numpy(rng.normal(size=(B, T))).cuda())[..., None].contiguous()
    k = K.Sum([K.Matern52(0.2, 1.0), K.Matern52(1.0, 0.5), K.Matern32(0.05, 0.2)])
    m = GaussianProcessRegression((t, y), k, torch.tensor([[0.1]], dtype=torch.float64, device="cuda"))
    return "b", "Sum(Matern52, Matern52, Matern32), B = 64", k, m, t, B


def run_case(make, cases, reps):
    from vidp_amd import hyper
    tag, name, k, m, t, B = make()
    d = k.state_dim
    kalman = m.posterior_kalman if hasattr(m, "posterior_kalman") else m._kalman
    pl = kalman.prior_ssm.plan
    dts = (t[:, 1:] - t[:, :-1]).contiguous()
    runs = {}
    if "kernel" in cases:
        _, mom, _ = kalman.log_likelihood_and_moments()
        kt = k._terms_struct()
        runs["kernel"] = lambda: pl.kernel_score(kt, dts, mom["x"], mom["Sig"], mom["Sub"])
    if "model" in cases:
        runs["log_likelihood"] = lambda: float(m.log_likelihood())
        runs["log_likelihood_and_grad"] = lambda: m.log_likelihood_and_grad()
    if "tape" in cases and tag == "a":
        def tape():
            elbo, leaves = m.classic_elbo_tape_hyper()
            return torch.autograd.grad(elbo, hyper.flatten(leaves))
        runs["classic_elbo_tape_hyper forward + backward"] = tape
    res = interleaved(runs, reps)
    pl.check_info()
    for variant, (ms, all_ms) in res.items():
        extra = {}
        if variant == "kernel":
            nbytes = B * (T * (d + d * (d + 1) // 2 + d * d) + (T - 1)) * 8
            extra = dict(algorithmic_bytes=nbytes, share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 4))
        emit(case=tag, model=name, d=d, B=B, T=T, variant=variant, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms], **extra)
    if "log_likelihood" in res:
        emit(case=tag, ratio="log_likelihood_and_grad / log_likelihood",
             value=round(res["log_likelihood_and_grad"][0] / res["log_likelihood"][0], 3))
    tp = "classic_elbo_tape_hyper forward + backward"
    if tp in res and "log_likelihood_and_grad" in res:
        emit(case=tag, ratio="tape forward + backward / log_likelihood_and_grad",
             value=round(res[tp][0] / res["log_likelihood_and_grad"][0], 3))
        g = hyper.flatten(m.log_likelihood_and_grad()[1])
        r = runs[tp]()
        emit(case=tag, check="native gradient against the tape's",
             max_rel_diff=max(abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(g, r)))
    del m, kalman, runs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="kernel,model,tape")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    cases = args.cases.split(",")
    for tag, make in (("a", case_a), ("b", case_b)):
        if args.only in ("", tag):
            run_case(make, cases, args.reps)


if __name__ == "__main__":
    main()
