"""Rates of the step mean function (vidp_amd.mean_function.StepMeanFunction): the native route (mfgm_action_coefficients: a segmented scan
in three launches; mfgm_action_mean: one launch; csrc/mfgm_mean.h) timed interleaved in one process against the torch route on the
same tensors (the reference's algorithm on existing pieces: transition_statistics_local, LowerTriangularBlockTriDiagonal(I, -A).solve,
searchsorted, gathers, a batched mat-vec):

    coefficients   from the perturbations to c: the solve against the generator, rhs = a_k-1 - a_k, the recurrence
    evaluation     H mu(t) at N unordered query points, the coefficients cached

Shape: K = N = 100 000 step actions on a jittered grid, query points uniform over the actions' span; d = 3 (Matern52) and d = 8
(Product(Matern32, HarmonicOscillator, HarmonicOscillator)), one chain and 64 chains.  Device-event timing; each repetition runs the
candidates one after the other, so that drift of the shared machine hits them alike; median, minimum and maximum over --reps
repetitions, one JSON line per candidate.  Algorithmic bytes: coefficients B K 8 (1 + 2 d) (times and rhs read, c written), evaluation
B N 8 (3 + 2 d) (the query point and the action time read, c and shift gathered, f written); `share_of_hbm_bound` is that over the HBM
peak over the median time -- a call time: it includes the launches and, for the coefficients, the torch glue of the right-hand side.

Kernel times come from a run of their own under the profiler, which this tool does not start:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mean_rate.py --kernels-only

runs every native candidate --reps times with nothing else in the process; the k_action_* rows of the stats table are the kernels.

    usage: python tools/mean_rate.py [--reps 30] [--K 100000] [--kernels-only]
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def kernel(d):
    from vidp_amd import kernels as K
    if d == 3:
        return K.Matern52(0.9, 1.2)
    return K.Product([K.Matern32(1.3, 0.8), K.HarmonicOscillator(0.9, 2.0), K.HarmonicOscillator(1.4, 3.1)])


def interleaved(cands, reps):
    """{name: [ms per repetition]}: every repetition times each candidate once, in turn."""
    for run in cands.values():
        run()
        run()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(reps):
        for name, run in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def case(d, B, K, reps, kernels_only):
    from vidp_amd.mean_function import StepMeanFunction
    rng = np.random.default_rng(d * 1000 + B)
    # a jittered grid over 150 time units: at most 75 periods of the shortest harmonic
    gaps = (150.0 / K) * (1.0 + 0.5 * rng.uniform(-1, 1, size=(B, K)))
    t = torch.from_numpy(np.cumsum(gaps, axis=-1)).cuda()
    u = torch.from_numpy(rng.normal(size=(B, K, d))).cuda()
    tq = torch.from_numpy(rng.uniform(0.0, 151.0, size=(B, K))).cuda()
    k = kernel(d)
    native, slow = StepMeanFunction(t, u, k), StepMeanFunction(t, u, k)
    slow._native = lambda device: None                     # the torch route on the same tensors
    assert native._native(t.device) is not None

    def coefficients(m):
        def run():
            m.kernel_changed()
            m._coefficients(t.device)
        return run

    cands = {"coefficients_native": coefficients(native), "evaluation_native": lambda: native(tq)}
    if kernels_only:
        for run in cands.values():
            for _ in range(reps):
                run()
        torch.cuda.synchronize()
        return
    cands.update({"coefficients_torch": coefficients(slow), "evaluation_torch": lambda: slow(tq)})
    times = interleaved(cands, reps)
    nbytes = {"coefficients": B * K * 8 * (1 + 2 * d), "evaluation": B * K * 8 * (3 + 2 * d)}
    launches = {"coefficients_native": "3 + rhs glue", "evaluation_native": 1}
    for name, ms in times.items():
        med = float(np.median(ms))
        what = name.split("_")[0]
        emit(case="rate", route=name, d=d, B=B, K=K, N=K, launches=launches.get(name, "torch ops"), ms_median=round(med, 5),
             ms_min=round(min(ms), 5), ms_max=round(max(ms), 5), reps=reps, algorithmic_bytes=nbytes[what],
             share_of_hbm_bound=round(nbytes[what] / HBM_PEAK / (med * 1e-3), 5))
    med = {n: float(np.median(ms)) for n, ms in times.items()}
    emit(case="ratio", d=d, B=B, K=K, coefficients_torch_over_native=round(med["coefficients_torch"] / med["coefficients_native"], 3),
         evaluation_torch_over_native=round(med["evaluation_torch"] / med["evaluation_native"], 3))
    # the two routes compute the same mean
    a, b = native(tq), slow(tq)
    emit(case="routes_agree", d=d, B=B, max_abs_diff=float((a - b).abs().max()), max_abs=float(b.abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--K", type=int, default=100_000)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mean_rate.py measures on the GPU; none found")
    for d in (3, 8):
        for B in (1, 64):
            case(d, B, args.K, args.reps, args.kernels_only)


if __name__ == "__main__":
    main()
