"""Gate of the pair route (DESIGN 5d follow-up): the parts of mfgm_cq_factor_pair timed alone, with HIP events, on the headline model's
own arrays, against the parts of the single route -- above all the forward-pair kernel against two lone forward sweeps.
usage: python tools/pair_gate.py [--B 64 --T 100000 --d 6 --reps 20]      prints one JSON line"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import vidp_amd  # noqa: E402
from vidp_amd.likelihoods import MultivariateGaussian  # noqa: E402
from vidp_amd.packed import _ptr, _stream  # noqa: E402
from vidp_amd.sde import DoubleWellSDE  # noqa: E402
from vidp_amd.variational_cvi_sde import CVISitesSDE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    B, T, d, dt, noise = a.B, a.T, a.d, 0.01, 0.1
    dev = torch.device("cuda:0")
    idx, ys = bench.synth_double_well(B, T, d, dt, 50, noise, seed=71892305 + 3)
    grid = np.arange(T) * dt
    m = CVISitesSDE(DoubleWellSDE(q=torch.eye(d, dtype=torch.float64)), grid, (grid[idx], torch.from_numpy(ys).to(dev)),
                    MultivariateGaussian(torch.from_numpy(bench.obs_chol(d, noise)).to(dev)), prior_initial_state=(np.zeros(d), np.eye(d)))
    m.pipe_pair = True
    for _ in range(3):                               # the loop as the bench runs it: the state, both factor buffers and a record exist
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.1)
        m.classic_elbo()
    pl, cq, lib = m.plan, m._cq, vidp_amd._lib.load()
    f, f2 = m._bufs["f"], m._bufs["f2"]
    cst, nxt = cq.struct(), cq.struct()
    nxt.site_lin, nxt.site_sym = m._ahead.bufs[0].data_ptr(), m._ahead.bufs[1].data_ptr()

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.reps

    def single(st):
        assert lib.mfgm_cq_factor_stage(pl.h, st, ctypes.byref(cst), _ptr(f["L"]), _ptr(f["y"]), _ptr(pl.ws), _ptr(pl.info), _stream()) == 0

    def pair(st):
        assert lib.mfgm_cq_factor_pair_stage(pl.h, st, ctypes.byref(cst), ctypes.byref(nxt), _ptr(f["L"]), _ptr(f["y"]), _ptr(f2["L"]),
                                             _ptr(f2["y"]), _ptr(pl.ws), _ptr(pl.info), _stream()) == 0

    # stage 0 of mfgm_cq_factor_pair_heads (one shared reduce + the two tails) where the model's observations allow it
    stride = m._pair_head_stride()
    scratch = pl._heads_scratch(stride) if stride else None

    def heads(st):
        assert lib.mfgm_cq_factor_pair_heads_stage(pl.h, st, stride, ctypes.byref(cst), ctypes.byref(nxt), _ptr(f["L"]), _ptr(f["y"]),
                                                   _ptr(f2["L"]), _ptr(f2["y"]), _ptr(scratch), scratch.numel(), _ptr(pl.ws), _ptr(pl.info),
                                                   _stream()) == 0

    klbuf = torch.empty(B, dtype=torch.float64, device=dev)

    def coarse_down():
        assert lib.mfgm_cq_selinv_kl(pl.h, 1, ctypes.byref(cst), _ptr(f["L"]), _ptr(f["y"]), ctypes.byref(m._sde_prm), None, None,
                                     _ptr(klbuf), None, None, _ptr(pl.ws), _stream()) == 0

    out = {}
    for rnd in (1, 2):                               # two alternating rounds: the spread between them is the noise of the figures
        out[f"round{rnd}"] = r = {
            "forward_alone_ms": timed(lambda: single(1)), "forward_pair_ms": timed(lambda: pair(1)),
            "reduce_alone_ms": timed(lambda: single(0)), "reduce_twice_ms": timed(lambda: pair(0)),
            "coarse_up_single_ms": timed(lambda: single(2)), "coarse_up_pair_ms": timed(lambda: pair(2)),
            "coarse_down_single_ms": timed(coarse_down), "coarse_down_pair_ms": timed(lambda: pair(3)),
        }
        if stride:
            r["reduce_heads_ms"] = timed(lambda: heads(0))
        r["pair_over_two_forwards"] = r["forward_pair_ms"] / (2.0 * r["forward_alone_ms"])
    pl.check_info()
    out["gate"] = "forward pair <= 0.89 x two lone forward sweeps"
    out["passes"] = bool(max(out[k]["pair_over_two_forwards"] for k in ("round1", "round2")) <= 0.89)
    out["config"] = dict(B=B, T=T, d=d, reps=a.reps, head_stride=stride, build=lib.mfgm_version().decode())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
