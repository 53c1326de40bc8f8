"""Rates of the LEG state-space build k_leg_ssm (mfgm_packed_leg_ssm, csrc/mfgm_leg_ssm.h), timed interleaved in one process against two
yardsticks on the same grid:

    leg         the new launch: one matrix exponential, Q, chol Q and offset per transition, outputs preallocated
    torch       the same kernel object through StationaryKernel._state_space_model_wide's steps on the torch transition statistics:
                torch.linalg.matrix_exp on [B (T-1), d, d], batched products and Cholesky -- what a user gets without the kernels
    floor       mfgm_packed_kernel_ssm on a Matern tree of the same d: the same stores with closed-form transitions

Shapes: T = 100 000, d = 3 and d = 8 (N = U[0, 1) + I, R = U[0, 1)), one chain and 64 chains, an irregular grid (gaps 0.01 (1 +- 0.1))
and a uniform one (every gap 0.01, on which a lane of k_leg_ssm evaluates one exponential and then only stores).  Device-event timing;
each repetition runs the candidates one after the other, so that drift of the shared machine hits them alike; median, minimum and
maximum over --reps repetitions, one JSON line per candidate.

Two bounds per shape.  Arithmetic: the fused multiply-adds the algorithm needs -- per evaluated transition (m - 1 + s) d^3 for the
Horner steps and squarings (m, s by the kernel's rule, restated here), d^2 for the first Horner step, d^2 (d + 1) / 2 for Q, d^2 for
the offset and d (d + 1) (d + 2) / 6 for the Cholesky factor; on the uniform grid a lane evaluates one transition per segment -- over
the fp64 vector peak (39.3e12 FMA/s).  Memory: the packed outputs written (A d^2, b d, chol Q d (d + 1) / 2 doubles per node) plus the
gaps read, over the HBM peak.  `share_of_bound` is the larger of the two least times over the median; `bound` names it.  The time
includes the launch, so at one chain it mostly measures launch overhead.

    usage: python tools/leg_rate.py [--reps 30] [--T 100000] [--torch-reps 30]
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
FMA_PEAK = 39.3e12       # fp64 vector FMA / s (78.6 TFLOP/s, MI355X spec)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def degree_and_squarings(theta):
    """(m, s) of leg_expm for theta = |F|_1 dt (arrays): s = 0 for theta <= 1/2 else ilogb(theta) + 2, m the smallest degree whose
    first dropped term (theta / 2^s)^(m+1) / (m+1)! is at most 1e-18 (capped at 18)."""
    theta = np.asarray(theta, dtype=np.float64)
    s = np.where(theta > 0.5, np.floor(np.log2(np.maximum(theta, 0.5))) + 2, 0).astype(np.int64)
    th = theta / 2.0 ** s
    m = np.ones_like(s)
    term = th.copy()
    live = np.ones(theta.shape, dtype=bool)
    for _ in range(17):
        term = np.where(live, term * th / (m + 1), term)
        live = live & (term > 1e-18)
        m = m + live
    return m, s


def fmas(d, m, s):
    return (m - 1 + s) * d ** 3 + d * d + d * d * (d + 1) // 2 + d * d + d * (d + 1) * (d + 2) // 6


def interleaved(cands, reps):
    """{name: [ms per repetition]}: every repetition times each candidate once, in turn (a candidate may ask for fewer repetitions)."""
    for run, _ in cands.values():
        run()
        run()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for i in range(reps):
        for name, (run, n) in cands.items():
            if i >= n:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def case(d, B, T, grid, reps, torch_reps):
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd._lib import FULL, TRI, VEC
    from vidp_amd.packed import Plan, _ptr, _stream
    lib = vidp_amd._lib.load()
    check = vidp_amd._lib.check
    rng = np.random.default_rng(d * 1000 + B)
    gk = K.LatentExponentiallyGenerated(rng.random((d, d)) + np.eye(d), rng.random((d, d)))
    gk.set_state_mean(rng.normal(size=d))
    if grid == "uniform":
        gaps = np.full((B, T - 1), 0.01)
    else:
        gaps = 0.01 * (1.0 + 0.1 * rng.uniform(-1, 1, size=(B, T - 1)))
    dts = torch.from_numpy(gaps).cuda()
    plan = Plan(B, T, d, device="cuda")
    out = (plan.empty(FULL), plan.empty(VEC), plan.empty(TRI))
    spec = gk._spec()
    matern = K.Matern52(0.3, 1.0) if d == 3 else K.Sum([K.Matern52(0.3, 1.0), K.Matern52(1.0, 0.5), K.Matern32(0.6, 0.8)])
    assert matern.state_dim == d
    kt = matern._terms_struct()

    def leg():
        check(lib.mfgm_packed_leg_ssm(plan.h, ctypes.byref(spec), _ptr(dts), *(_ptr(o) for o in out), _ptr(plan.info), _stream()), "leg")

    def floor():
        check(lib.mfgm_packed_kernel_ssm(plan.h, ctypes.byref(kt), _ptr(dts), *(_ptr(o) for o in out), _ptr(plan.info), _stream()), "floor")

    mean = gk.state_mean.cuda()
    P0 = gk.initial_covariance_matrix().cuda()

    def torch_route():
        # StationaryKernel._state_space_model_wide on the base class's transition statistics, i.e. on _parts' torch.linalg.matrix_exp
        # (_state_space_model_wide itself would call gk.transition_statistics_local, which is the HIP k_leg_transitions here)
        A, Q = K.StationaryKernel.transition_statistics_local(gk, dts)
        return K._model_from_torch(A, Q, mean, mean, P0, plan, (B,))

    times = interleaved({"leg": (leg, reps), "torch": (torch_route, torch_reps), "floor": (floor, reps)}, reps)
    plan.check_info()
    # the two routes build the same model
    A, off, chol = plan.leg_ssm(spec, dts)
    ref = torch_route()
    diff = max(float((plan.unpack(FULL, A, T - 1) - ref.state_transitions).abs().max()),
               float((plan.unpack(VEC, off)[:, 1:] - ref.state_offsets).abs().max()),
               float((plan.unpack(TRI, chol)[:, 1:] - ref.cholesky_process_covariances).abs().max()))
    theta = float(gk.feedback_matrix.abs().sum(dim=0).max()) * gaps
    m, s = degree_and_squarings(theta if grid == "irregular" else theta[:1, :1])
    per = fmas(d, m, s)
    if grid == "uniform":
        nfma = float(per.mean()) * B * plan.P          # one evaluation per lane (segment)
    else:
        nfma = float(per.sum()) * (1.0 + plan.P / T)   # len + 1 transitions per lane
    nbytes = B * T * 8 * (d * d + d + d * (d + 1) // 2 + 1)
    t_fma, t_mem = nfma / FMA_PEAK, nbytes / HBM_PEAK
    for name, ms in times.items():
        med = float(np.median(ms))
        row = dict(case="rate", route=name, d=d, B=B, T=T, grid=grid, ms_median=round(med, 5), ms_min=round(min(ms), 5),
                   ms_max=round(max(ms), 5), reps=len(ms), algorithmic_bytes=nbytes, share_of_hbm_bound=round(t_mem / (med * 1e-3), 4))
        if name == "leg":
            row.update(degree_mean=round(float(m.mean()), 2), squarings_max=int(s.max()), fma=nfma,
                       share_of_fma_bound=round(t_fma / (med * 1e-3), 4), bound="fp64 issue" if t_fma > t_mem else "HBM",
                       share_of_bound=round(max(t_fma, t_mem) / (med * 1e-3), 4))
        emit(**row)
    med = {k: float(np.median(v)) for k, v in times.items()}
    emit(case="ratio", d=d, B=B, T=T, grid=grid, leg_over_torch=round(med["leg"] / med["torch"], 5),
         leg_over_floor=round(med["leg"] / med["floor"], 4), leg_max_over_torch_min=round(max(times["leg"]) / min(times["torch"]), 5),
         routes_max_abs_diff=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--torch-reps", type=int, default=30)
    ap.add_argument("--T", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/leg_rate.py measures on the GPU; none found")
    for d in (3, 8):
        for B in (1, 64):
            for grid in ("irregular", "uniform"):
                case(d, B, args.T, grid, args.reps, min(args.torch_reps, args.reps))
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
