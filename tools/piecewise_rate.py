"""Rates of the piecewise-stationary SSM build k_piecewise_ssm (mfgm_packed_piecewise_ssm, csrc/mfgm_piecewise_ssm.h), timed interleaved in
one process against two yardsticks on the same grid:

    piecewise   the new launch: 6 regions, the kernel looks the regions up itself, outputs preallocated
    floor       mfgm_packed_kernel_ssm on region 0's terms at the same shape: the same stores without the region lookup
    reference   the reference's algorithm on top of the existing kernel: partition the transitions by the region of their left end (a
                host synchronisation sizes the parts), one mfgm_packed_kernel_ssm launch per region on a plan of the part's size,
                concatenation of the parts in natural layout, packing into the chain's layout (one chain only)

Shapes: T = 100 000, d = 3 (Matern52, 6 regions: the piecewise notebook's configuration scaled up) and d = 8
(Product(HarmonicOscillator, Matern32, HarmonicOscillator)), one chain and 64 chains.  Device-event timing; each repetition runs the
candidates one after the other, so that drift of the shared machine hits them alike; median, minimum and maximum over --reps
repetitions, one JSON line per candidate.  Algorithmic bytes: the packed outputs written (A d^2, b d, chol Q d (d + 1) / 2 doubles per
node) plus the time points read; `share_of_hbm_bound` is that over the HBM peak over the median time -- the time includes the launch,
so at one chain it is a measurement of launch overhead, not of the kernel.  Also reports whether one region gives bit-identical arrays
through both entry points.

    usage: python tools/piecewise_rate.py [--reps 30] [--T 100000]
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def children(d, n):
    from vidp_amd import kernels as K
    ls = [0.3, 1.0, 0.2, 0.6, 1.5, 0.4][:n]
    if d == 3:
        return [K.Matern52(l, 1.0 + 0.1 * i) for i, l in enumerate(ls)]
    return [K.Product([K.HarmonicOscillator(1.0 + 0.1 * i, 3.0 * l), K.Matern32(1.5 * l, 0.8), K.HarmonicOscillator(0.5, 0.7 * l)])
            for i, l in enumerate(ls)]


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


def case(d, B, T, reps):
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd._lib import FULL, TRI, VEC
    from vidp_amd.packed import Plan, _ptr, _stream
    lib = vidp_amd._lib.load()
    rng = np.random.default_rng(d * 1000 + B)
    gaps = 0.01 * (1.0 + 0.1 * rng.uniform(-1, 1, size=(B, T - 1)))
    t = torch.from_numpy(np.concatenate([np.zeros((B, 1)), np.cumsum(gaps, axis=-1)], axis=-1)).cuda()
    dts = (t[:, 1:] - t[:, :-1]).contiguous()
    kids = children(d, 6)
    cp = np.linspace(0.0, 0.01 * T, 7)[1:-1]
    pk = K.PiecewiseKernel(kids, cp)
    plan = Plan(B, T, d, device="cuda")
    out = (plan.empty(FULL), plan.empty(VEC), plan.empty(TRI))
    pw, tab = pk._terms_struct(t.device)
    kt = kids[0]._terms_struct()
    check = vidp_amd._lib.check

    def piecewise():
        check(lib.mfgm_packed_piecewise_ssm(plan.h, ctypes.byref(pw), _ptr(t), *(_ptr(o) for o in out), _ptr(plan.info), _stream()), "piecewise")

    def floor():
        check(lib.mfgm_packed_kernel_ssm(plan.h, ctypes.byref(kt), _ptr(dts), *(_ptr(o) for o in out), _ptr(plan.info), _stream()), "floor")

    cands = {"piecewise": piecewise, "floor": floor}
    plans = {}

    def reference():
        # one chain: the parts of a sorted grid are contiguous, so the concatenation of the parts is the chain (the reference's tf.concat)
        region = pk.split_time_indices(t[0, :-1])
        sizes = torch.bincount(region, minlength=len(kids)).tolist()          # the host synchronisation of dynamic_partition
        As, offs, chols, lo = [], [], [], 0
        for i, n in enumerate(sizes):
            if n == 0:
                continue
            pl = plans.setdefault(n, Plan(1, n + 1, d, device="cuda"))
            A, off, chol = pl.kernel_ssm(kids[i]._terms_struct(), dts[:, lo:lo + n].contiguous())
            if lo == 0:
                offs.append(torch.zeros((1, 1, d), dtype=torch.float64, device="cuda"))
                chols.append(pl.unpack(TRI, chol)[:, :1])
            As.append(pl.unpack(FULL, A, n))
            offs.append(pl.unpack(VEC, off)[:, 1:])
            chols.append(pl.unpack(TRI, chol)[:, 1:])
            lo += n
        return plan.pack(FULL, torch.cat(As, dim=1)), plan.pack(VEC, torch.cat(offs, dim=1)), plan.pack(TRI, torch.cat(chols, dim=1))

    if B == 1:
        cands["reference"] = reference
    times = interleaved(cands, reps)
    plan.check_info()
    nbytes = B * T * 8 * (d * d + d + d * (d + 1) // 2 + 1)
    for name, ms in times.items():
        med = float(np.median(ms))
        emit(case="rate", route=name, d=d, B=B, T=T, regions=6, launches={"piecewise": 1, "floor": 1}.get(name, "6 + glue"),
             ms_median=round(med, 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5), reps=reps, algorithmic_bytes=nbytes,
             share_of_hbm_bound=round(nbytes / HBM_PEAK / (med * 1e-3), 4))
    if B == 1:
        emit(case="ratio", d=d, B=B, T=T, piecewise_over_reference=round(float(np.median(times["piecewise"]) / np.median(times["reference"])), 4),
             piecewise_over_floor=round(float(np.median(times["piecewise"]) / np.median(times["floor"])), 4))
        # the two routes build the same model
        nat = lambda p: (plan.unpack(FULL, p[0], T - 1), plan.unpack(VEC, p[1]), plan.unpack(TRI, p[2]))
        a, b = nat(plan.piecewise_ssm(pw, t)), nat(reference())
        emit(case="routes_agree", d=d, max_abs_diff=float(max((x - y).abs().max() for x, y in zip(a, b))))
        one = K.PiecewiseKernel(kids[:1], [])
        pw1, tab1 = one._terms_struct(t.device)
        a, b = nat(plan.piecewise_ssm(pw1, t)), nat(plan.kernel_ssm(kt, dts))
        plan.check_info()
        emit(case="one_region_both_entry_points", d=d, bit_identical=bool(all(torch.equal(x, y) for x, y in zip(a, b))),
             max_abs_diff=float(max((x - y).abs().max() for x, y in zip(a, b))))
    else:
        emit(case="ratio", d=d, B=B, T=T, piecewise_over_floor=round(float(np.median(times["piecewise"]) / np.median(times["floor"])), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--T", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/piecewise_rate.py measures on the GPU; none found")
    for d in (3, 8):
        for B in (1, 64):
            case(d, B, args.T, args.reps)


if __name__ == "__main__":
    main()
