"""Rates of the sparse-CVI hyper-parameter gradient: SparseCVIGaussianProcess.elbo_and_grad on the HIP route
against the torch route of the same object (VIDP_NATIVE_SPARSE_SCORE=0) and against `update_sites; classic_elbo` of the same model, and
the entry point mfgm_sparse_cond_score (csrc/mfgm_sparse_score.h) alone (variant "kernel": an event time over its memset and two
launches).  M = 200 000 inducing states 0.1 apart, N = 400 000 sorted observations:

    a   Matern-5/2 (d = 3), Gaussian likelihood
    b   Sum(Matern52, Matern52, Matern32) (d = 8), Gaussian likelihood
    c   Matern-5/2 (d = 3), Bernoulli labels

Device-event timing; the variants of a case are INTERLEAVED (one run of each per repetition, in one process) and the median of --reps
repetitions is reported, one JSON line per variant.  The kernel's algorithmic bytes are (2 d + 4) 8 per observation (w, the two gaps,
a, b) plus (d + 2 d^2) 8 per inducing state (the marginals, read once), reported as a share of the 8 TB/s peak.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats -- python tools/sparse_hyper_rate.py --cases kernel` run.

    usage: python tools/sparse_hyper_rate.py [--reps 30] [--cases kernel,model,torch] [--only a|b|c]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.hyper_rate import HBM_PEAK, emit, interleaved  # noqa: E402

M, N = 200_000, 400_000


def make(tag):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    rng = np.random.default_rng(71892305 + 21)
    z = torch.linspace(0.0, 0.1 * (M - 1), M, dtype=torch.float64, device="cuda")
    t = torch.from_numpy(np.sort(rng.uniform(-0.05, 0.1 * (M - 1) + 0.05, N))).cuda()
    f = torch.sin(3 * t) + 0.1 * torch.from_numpy(rng.normal(size=N)).cuda()
    if tag == "b":
        k, name = K.Sum([K.Matern52(0.5, 1.0), K.Matern52(2.0, 0.5), K.Matern32(0.3, 0.2)]), "Sum(Matern52, Matern52, Matern32)"
    else:
        k, name = K.Matern52(0.5, 1.0), "Matern52"
    if tag == "c":
        lik, y, name = Bernoulli(1e-3), (f > 0).to(torch.float64), name + ", Bernoulli"
    else:
        lik, y, name = Gaussian(0.01), f, name + ", Gaussian"
    m = SparseCVIGaussianProcess(k, z, lik, learning_rate=0.5)
    data = (t, y[:, None].contiguous())
    for _ in range(2):
        m.update_sites(data)
    return name, k, m, data


def run_case(tag, cases, reps):
    from vidp_amd import hyper
    from vidp_amd.conditionals import interval_gaps
    name, k, m, data = make(tag)
    d = k.state_dim
    pl = m.dist_p.plan
    runs = {}
    if "kernel" in cases:
        dd = m._data(data)
        marg = m._marginals()
        _, glo, ghi = interval_gaps(data[0], m.inducing_inputs)
        fmu, fvar = m._predict_f_data(dd)
        g1, g2 = m.likelihood.ve_gradients_expectation(fmu, fvar, data[1])
        a = (g1 + 2.0 * g2 * fmu).reshape(-1).contiguous()
        b = g2.reshape(-1).contiguous()
        runs["kernel"] = lambda: hyper.conditional_part_native(k, pl, dd, glo, ghi, a, b, marg)
    if "model" in cases:
        def step():
            m.update_sites(data)
            return float(m.classic_elbo(data))
        runs["update_sites + classic_elbo"] = step
        runs["elbo_and_grad (HIP route)"] = lambda: m.elbo_and_grad(data)
    if "torch" in cases:
        def torch_route():
            os.environ["VIDP_NATIVE_SPARSE_SCORE"] = "0"
            try:
                return m.elbo_and_grad(data)
            finally:
                del os.environ["VIDP_NATIVE_SPARSE_SCORE"]
        runs["elbo_and_grad (torch route)"] = torch_route
    if "parts" in cases:
        # where the HIP route's time goes: the chain part is the Fisher-vector product plus one score launch
        from vidp_amd import tape
        T = m.dist_p.T
        m._theta()
        tb, mg = m._theta_bufs, m._marginals()
        v = [torch.randn_like(mg["mu"])[None], torch.randn_like(mg["Sig"])[None], torch.randn_like(mg["Sub"][:T - 1])[None]]
        runs["fisher_vector_product"] = lambda: tape.fisher_vector_product(pl, tb["diag"][None], tb["sub"][None, :T - 1], mg["mu"][None],
                                                                           mg["Sig"][None], mg["Sub"][None, :T - 1], *v)
    res = interleaved(runs, reps)
    pl.check_info()
    for variant, (ms, all_ms) in res.items():
        extra = {}
        if variant == "kernel":
            nbytes = (N * (2 * d + 4) + M * (d + 2 * d * d)) * 8
            extra = dict(algorithmic_bytes=nbytes, share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 4))
        emit(case=tag, model=name, d=d, M=M, N=N, variant=variant, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms], **extra)
    hip, tr, st = "elbo_and_grad (HIP route)", "elbo_and_grad (torch route)", "update_sites + classic_elbo"
    if hip in res and st in res:
        emit(case=tag, ratio="elbo_and_grad (HIP route) / (update_sites + classic_elbo)", value=round(res[hip][0] / res[st][0], 3))
    if hip in res and tr in res:
        emit(case=tag, ratio="torch route / HIP route", value=round(res[tr][0] / res[hip][0], 3))
        g, r = hyper.flatten(runs[hip]()[1]), hyper.flatten(runs[tr]()[1])
        emit(case=tag, check="HIP route against the torch route",
             max_rel_diff=max(abs(float(x) - float(y)) / max(1.0, abs(float(y))) for x, y in zip(g, r)))
    del m, runs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="kernel,model,torch,parts")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    cases = args.cases.split(",")
    for tag in ("a", "b", "c"):
        if args.only in ("", tag):
            run_case(tag, cases, args.reps)


if __name__ == "__main__":
    main()
