"""Rates of mini-batch sparse CVI: SparseCVIGaussianProcess(num_data=) on unsorted batches, the native route (one
launch of mfgm_sparse_batch_predict_lik per step, csrc/mfgm_minibatch.h) against the torch route of the same object
(VIDP_NATIVE_MINIBATCH=0).  M = 20 000 inducing states 0.1 apart, a data set of num_data = 2 000 000 points, batches of 4 096 and
65 536 points drawn from it -- a NEW tensor every step, as a trainer hands them over (neither route can reuse anything):

    a   Matern-5/2 (d = 3), Poisson counts
    b   Sum(Matern52, Matern52, Matern32) (d = 8), Bernoulli labels

Variants, INTERLEAVED (one run of each per repetition, in one process; device-event timing; the median of --reps repetitions, one JSON
line per variant):

    update_sites / update_sites; classic_elbo      on the native and on the torch route
    factorisation                                  _marginals() alone: the factorisation and selected inverse that every update_sites
                                                   above begins with on either route (classic_elbo after it makes a second one)
    kernel                                         the entry point alone on the step's arrays (its launch and the fixed-order sum of ve)
    full batch                                     for context: update_sites; classic_elbo of a model without num_data on the whole sorted
                                                   data set (its constants cached, as that route keeps them)

The kernel's algorithmic bytes are (2 d + 8) 8 per point (t and y read; w, c, fmu, fvar, ve, g1, g2 written) plus (1 + d + 2 d^2) 8 per
inducing state (z and the marginals, read once), reported as a share of the 8 TB/s peak.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/minibatch_rate.py --cases kernel` run.

    usage: python tools/minibatch_rate.py [--reps 30] [--cases model,kernel,full] [--only a|b] [--batches 4096,65536]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.hyper_rate import HBM_PEAK, emit, interleaved  # noqa: E402

M, NUM_DATA = 20_000, 2_000_000


def make(tag):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Poisson
    rng = np.random.default_rng(71892305 + 26)
    z = torch.linspace(0.0, 0.1 * (M - 1), M, dtype=torch.float64, device="cuda")
    t = torch.from_numpy(np.sort(rng.uniform(-0.05, 0.1 * (M - 1) + 0.05, NUM_DATA))).cuda()
    f = 0.8 * torch.sin(3 * t) + 0.1 * torch.from_numpy(rng.normal(size=NUM_DATA)).cuda()
    if tag == "b":
        k, name = K.Sum([K.Matern52(0.5, 1.0), K.Matern52(2.0, 0.5), K.Matern32(0.3, 0.2)]), "Sum(Matern52, Matern52, Matern32), Bernoulli"
        lik, y = Bernoulli(1e-3), (f > 0).to(torch.float64)
    else:
        k, name = K.Matern52(0.5, 1.0), "Matern52, Poisson"
        lik, y = Poisson(1.0), torch.poisson(torch.exp(f))
    return name, k, lik, z, (t, y[:, None].contiguous())


class Batches:
    """Unsorted batches of n points of the data set, each a new pair of tensors handed out once; drawn before the timed window."""

    def __init__(self, data, n, count, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        t, y = data
        self.items = []
        for _ in range(count):
            sel = torch.randint(0, t.shape[0], (n,), generator=g, device="cuda")
            self.items.append((t[sel].contiguous(), y[sel].contiguous()))
        self.at = 0

    def next(self):
        b = self.items[self.at]
        self.at += 1
        return b


def torch_route(fn):
    def run():
        os.environ["VIDP_NATIVE_MINIBATCH"] = "0"
        try:
            return fn()
        finally:
            del os.environ["VIDP_NATIVE_MINIBATCH"]
    return run


def run_case(tag, cases, reps, sizes):
    from vidp_amd import _lib
    from vidp_amd.packed import _ptr, _stream
    from vidp_amd.sparse_variational_cvi import _BATCH_KINDS, SparseCVIGaussianProcess
    name, k, lik, z, data = make(tag)
    d = k.state_dim
    for n in sizes:
        # rho = n / num_data: the step a 1 / k schedule reaches after one epoch; every batch point then enters with weight rho scale = 1
        m = SparseCVIGaussianProcess(k, z, lik, learning_rate=n / NUM_DATA, num_data=NUM_DATA)
        src = Batches(data, n, 6 * (reps + 1) + 4, seed=n)          # two steps per repetition take two each
        for _ in range(3):
            m.update_sites(src.next())
        assert m._batch_native(data[0])
        pl = m.dist_p.plan
        runs = {}
        if "model" in cases:
            def sites():
                m.update_sites(src.next())

            def step():
                b = src.next()
                m.update_sites(b)
                return m.classic_elbo(b)

            def factor():
                m._marg = None
                m._marginals()
                m._marg = None          # (the next variant's update_sites makes its own, as after any step)
            runs["update_sites (native)"] = sites
            runs["update_sites (torch route)"] = torch_route(sites)
            runs["update_sites; classic_elbo (native)"] = step
            runs["update_sites; classic_elbo (torch route)"] = torch_route(step)
            runs["factorisation"] = factor
        if "kernel" in cases:
            c = m._batch_pass(src.next())
            seg, w, out, ts, ys, shift = c["keep"]
            kc, marg = m._batch_consts, m._marginals()
            ws = torch.empty(int(pl.lib.mfgm_sparse_batch_workspace_doubles(n)), dtype=torch.float64, device="cuda")
            kind = _BATCH_KINDS[type(lik)]

            def kernel():
                _lib.check(pl.lib.mfgm_sparse_batch_predict_lik(ctypes.byref(kc["terms"]), M, _ptr(kc["z"]), n, _ptr(ts), None, kind,
                                                                float(lik.param), NUM_DATA / n, _ptr(ys), _ptr(kc["init"][0]),
                                                                _ptr(kc["init"][1]), _ptr(marg["mu"]), _ptr(marg["Sig"]), _ptr(marg["Sub"]), None,
                                                                _ptr(w), *(_ptr(o) for o in out), _ptr(c["ve_sum"]), _ptr(ws), _ptr(pl.info),
                                                                _stream()), "mfgm_sparse_batch_predict_lik")
            runs["kernel"] = kernel
        res = interleaved(runs, reps)
        pl.check_info()
        for variant, (ms, all_ms) in res.items():
            extra = {}
            if variant == "kernel":
                nbytes = (n * (2 * d + 8) + M * (1 + d + 2 * d * d)) * 8
                extra = dict(algorithmic_bytes=nbytes, share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 5))
            emit(case=tag, model=name, d=d, M=M, num_data=NUM_DATA, batch=n, variant=variant, ms=round(ms, 4),
                 ms_all=[round(x, 4) for x in all_ms], **extra)
        for what in ("update_sites", "update_sites; classic_elbo"):
            a, b = f"{what} (native)", f"{what} (torch route)"
            if a in res:
                emit(case=tag, batch=n, ratio=f"{what}: torch route / native", value=round(res[b][0] / res[a][0], 3))
                emit(case=tag, batch=n, ratio=f"factorisation / {what} (native)", value=round(res["factorisation"][0] / res[a][0], 3))
        del m, runs
        torch.cuda.empty_cache()
    if "full" in cases:
        full = SparseCVIGaussianProcess(k, z, lik, learning_rate=0.05)
        for _ in range(2):
            full.update_sites(data)

        def full_step():
            full.update_sites(data)
            return full.classic_elbo(data)
        ms, all_ms = interleaved({"full": full_step}, max(3, reps // 3))["full"]
        emit(case=tag, model=name, d=d, M=M, N=NUM_DATA, variant="full batch, sorted: update_sites; classic_elbo", ms=round(ms, 4),
             ms_all=[round(x, 4) for x in all_ms])
        del full
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="model,kernel,full")
    ap.add_argument("--only", default="")
    ap.add_argument("--batches", default="4096,65536")
    args = ap.parse_args()
    for tag in ("a", "b"):
        if args.only in ("", tag):
            run_case(tag, args.cases.split(","), args.reps, [int(s) for s in args.batches.split(",")])


if __name__ == "__main__":
    main()
