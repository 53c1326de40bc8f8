"""Rates of the Euler-Maruyama kernel (sde_utils.euler_maruyama, csrc/mfgm_sim.h) on three shapes:

    a  double well, d = 1, B = 65 536 paths, N = 1 001    (many paths: against the bytes-written bound)
    b  double well, d = 6, B = 64, N = 100 001            (one wave: latency per step)
    c  Van der Pol, d = 2, B = 4 096, N = 10 001

Device-event timing after a warm-up; one JSON line per shape.  `--stage-ab 0,8,32` times shape a with each staging depth
(MFGM_EM_STAGE, read once per process) in fresh child processes, alternating the depths over `--rounds` rounds.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/em_rate.py` run.

    usage: python tools/em_rate.py [--configs a,b,c] [--reps 5] [--stage-ab 0,8,16,32 --rounds 2]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s (MI355X spec)
CLOCK = 2.4e9            # Hz, the MI355X's top clock (cycles per step below are at this clock)

SHAPES = {"a": ("dw", 1, 65_536, 1_001), "b": ("dw", 6, 64, 100_001), "c": ("vanderpol", 2, 4_096, 10_001)}


def make(name, d):
    from vidp_amd import sde as S
    q = torch.eye(d, dtype=torch.float64)
    return S.DoubleWellSDE(q=q) if name == "dw" else S.VanderPolOscillatorSDE(a=2.0, tau=5.0, q=q)


def time_shape(key, reps):
    from vidp_amd.sde_utils import euler_maruyama
    name, d, B, N = SHAPES[key]
    sde = make(name, d)
    dt = 0.01 if name == "dw" else 0.002
    tg = torch.arange(1, N + 1, dtype=torch.float64, device="cuda") * dt
    x0 = torch.zeros(B, d, dtype=torch.float64, device="cuda")
    run = lambda: euler_maruyama(sde, x0, tg, seed=1, native=True)
    X = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(X).all())
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    t = sorted(times)[len(times) // 2]
    nbytes = B * N * d * 8
    normals = B * (N - 1) * d
    return dict(shape=key, sde=name, d=d, B=B, N=N, stage=os.environ.get("MFGM_EM_STAGE", "default"), ms=round(t * 1e3, 4),
                ms_all=[round(x * 1e3, 4) for x in times], bytes_written=nbytes, write_bound_ms=round(nbytes / HBM_PEAK * 1e3, 4),
                share_of_write_bound=round(nbytes / HBM_PEAK / t, 4), normals_per_s=normals / t, ns_per_step=round(t / (N - 1) * 1e9, 2),
                cycles_per_step_at_2p4GHz=round(t / (N - 1) * CLOCK, 1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="a,b,c")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--stage-ab", default="")
    p.add_argument("--rounds", type=int, default=2)
    a = p.parse_args()
    if a.stage_ab:
        for r in range(a.rounds):
            for s in a.stage_ab.split(","):
                env = dict(os.environ, MFGM_EM_STAGE=s)
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--configs", "a", "--reps", str(a.reps)], env=env,
                                    timeout=600).returncode
                if rc != 0:
                    print(json.dumps({"error": f"stage {s} exited with {rc}"}))
                    sys.exit(1)
        return
    for key in a.configs.split(","):
        print(json.dumps(time_shape(key, a.reps)), flush=True)


if __name__ == "__main__":
    main()
