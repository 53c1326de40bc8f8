"""Rates of the term kernel k_kernel_ssm (mfgm_packed_kernel_ssm, csrc/mfgm_kernel_ssm.h) and of a CVI-GP step on a quasi-periodic prior:

    kernel   k_kernel_ssm<6> for Product(Matern52, HarmonicOscillator) and k_stationary_ssm<6> for Sum(Matern52, Matern52) on the same
             grid (B = 64, T = 100 000, spacing 0.01), outputs preallocated; both write 504 B per node (A 36, b 6, chol Q 21 doubles).
             Also reports whether a Matern-only tree gives bit-identical arrays through the two entry points.
    step     config 2's CVI-GP model (T = 100 000, one chain, Gaussian likelihood; bench.py c2) with the quasi-periodic priors
             Product(Matern32, HarmonicOscillator) (d = 4) and Product(Matern52, HarmonicOscillator) (d = 6): one step_graph() replay,
             and config 2's own Matern-5/2 prior (d = 3) as the yardstick

Device-event timing, median of --reps runs after a warm-up; one JSON line per case.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/kernel_rate.py --cases kernel` run.

    usage: python tools/kernel_rate.py [--reps 20] [--cases kernel,step]
"""
import argparse
import ctypes
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
    from vidp_amd import kernels as K
    from vidp_amd._lib import FULL, TRI, VEC
    from vidp_amd.packed import Plan, _ptr, _stream
    lib = vidp_amd._lib.load()
    B, T, d = 64, 100_000, 6
    plan = Plan(B, T, d, device="cuda")
    rng = np.random.default_rng(0)
    dts = torch.from_numpy(0.01 * (1.0 + 0.1 * rng.uniform(-1, 1, size=(B, T - 1)))).cuda()
    out = (plan.empty(FULL), plan.empty(VEC), plan.empty(TRI))
    qp = K.Product([K.Matern52(0.5, 1.0), K.HarmonicOscillator(1.0, 0.7)])
    mm = K.Sum([K.Matern52(0.5, 1.0), K.Matern52(2.0, 0.5)])
    kt, spec = qp._terms_struct(), mm._spec()
    calls = {
        "k_kernel_ssm<6> Product(Matern52, HarmonicOscillator)":
            lambda: lib.mfgm_packed_kernel_ssm(plan.h, ctypes.byref(kt), _ptr(dts), *(_ptr(o) for o in out), _ptr(plan.info), _stream()),
        "k_stationary_ssm<6> Sum(Matern52, Matern52)":
            lambda: lib.mfgm_packed_stationary_ssm(plan.h, ctypes.byref(spec), _ptr(dts), *(_ptr(o) for o in out), _ptr(plan.info),
                                                   _stream()),
        "k_kernel_ssm<6> Sum(Matern52, Matern52)":
            lambda: lib.mfgm_packed_kernel_ssm(plan.h, ctypes.byref(mm._terms_struct()), _ptr(dts), *(_ptr(o) for o in out),
                                               _ptr(plan.info), _stream()),
    }
    res = {}
    for name, call in calls.items():
        def run():
            vidp_amd._lib.check(call(), name)
        ms, all_ms = timed(run, reps)
        plan.check_info()
        nbytes = B * T * 504
        res[name] = ms
        emit(case="kernel", kernel=name, B=B, T=T, ms=round(ms, 5), ms_all=[round(x, 5) for x in all_ms], bytes_written=nbytes,
             share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 4))
    names = list(calls)
    emit(case="kernel_ratio", ratio=round(res[names[0]] / res[names[1]], 4), what=f"{names[0]} / {names[1]}")
    # natural layout: the padding of the packed layout is never written
    nat = lambda p: (plan.unpack(FULL, p[0], T - 1), plan.unpack(VEC, p[1]), plan.unpack(TRI, p[2]))
    a = nat(plan.stationary_ssm(spec, dts))
    b = nat(plan.kernel_ssm(mm._terms_struct(), dts))
    plan.check_info()
    emit(case="matern_tree_both_entry_points", kernel="Sum(Matern52, Matern52)",
         bit_identical=bool(all(torch.equal(x, y) for x, y in zip(a, b))),
         max_abs_diff=float(max((x - y).abs().max() for x, y in zip(a, b))))


def step_cases(reps):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    T = 100_000
    rng = np.random.default_rng(71892305 + 2)
    t = torch.linspace(0, 0.01 * T, T, dtype=torch.float64, device="cuda")
    y = (torch.sin(12 * t) + 0.1 * torch.from_numpy(rng.normal(size=T)).cuda())[:, None].contiguous()
    priors = {"Matern52 (config 2)": lambda: K.Matern52(lengthscale=0.2, variance=1.0),
              "Product(Matern32, HarmonicOscillator)": lambda: K.Product([K.Matern32(0.5, 1.0), K.HarmonicOscillator(1.0, 0.52)]),
              "Product(Matern52, HarmonicOscillator)": lambda: K.Product([K.Matern52(0.5, 1.0), K.HarmonicOscillator(1.0, 0.52)])}
    for name, mk in priors.items():
        k = mk()
        m = CVIGaussianProcess((t, y), k, Gaussian(0.01), learning_rate=0.5)
        step = m.step_graph()
        ms, all_ms = timed(step, reps)
        emit(case="step", prior=name, d=k.state_dim, route="graph", T=T, ms=round(ms, 4), ms_all=[round(x, 4) for x in all_ms],
             elbo=float(step()))
        del m, step
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
