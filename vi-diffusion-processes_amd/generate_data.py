"""
Experiment data of the diffusion-process workflow (docs/diffusion_processes/generate_data.py:22-49 and its command line, without the
plotting and the k-fold split): an SDE path simulated by `sde_utils.euler_maruyama`, observed with Gaussian noise at a random subset of the
grid, plus a held-out test subset, written as the reference's `.npz` (read back by `exp_io.load_exp_data`).

    python -m vidp_amd.generate_data -sde ou -d 0.5 -q 0.8 -t0 0 -t1 10 -x0 0 -dt 0.01 -n 30 -o data

(from the repository root).  The latent path comes from the counter-based stream with the given seed; the observation and test grids
(sizes n and int(0.2 n), drawn without replacement and sorted) and the observation noise from numpy.random.default_rng(seed).
"""
import argparse
import os

import numpy as np

SDES = ("ou", "dw", "benes", "sine", "sqrt", "vanderpol")


def build_parser():
    p = argparse.ArgumentParser(prog="python -m vidp_amd.generate_data", description="Generate observations from an SDE.")
    p.add_argument("-sde", help="SDE to simulate the process", choices=SDES, required=True)
    p.add_argument("-d", "--decay", help="Decay for the Ornstein-Uhlenbeck process.", default=0.5, type=float)
    p.add_argument("-q", "--diffusion", help="Spectral density for the diffusion process.", type=float, default=0.8)
    p.add_argument("-t0", help="Time t0.", type=float, default=0.0)
    p.add_argument("-t1", help="Time t1.", type=float, default=1.0)
    p.add_argument("-x0", help="State at t0.", type=float, default=0.0)
    p.add_argument("-dt", help="Time step value (dt)", type=float, default=0.01)
    p.add_argument("-n", "--num_observations", help="Number of Observations", type=int, default=10)
    p.add_argument("-si", "--sigma", help="Noise std-deviation", type=float, default=0.1)
    p.add_argument("-o", "--output", help="Output directory path.", type=str, default="")
    p.add_argument("-s", "--seed", help="Set the seed.", type=int, default=33)
    p.add_argument("-dim", help="Number of state dimensions.", type=int, default=1)
    return p


def time_grid_of(t0, t1, dt):
    """The reference's grid: range(t0, t1 + dt, dt) rounded to the decimals of dt."""
    n_decimals = str(dt)[::-1].find(".")
    return np.round(np.arange(t0, t1 + dt, dt, dtype=np.float64), decimals=n_decimals)


def parse_args(argv=None):
    """Parse and check the command line (no GPU needed); errors exit through argparse with status 2."""
    p = build_parser()
    a = p.parse_args(argv)
    if not a.dt > 0:
        p.error(f"-dt must be positive, got {a.dt}")
    if a.t0 < 0 or a.t1 < a.t0:
        p.error(f"need 0 <= t0 <= t1, got t0={a.t0}, t1={a.t1}")
    if a.dim < 1:
        p.error(f"-dim must be at least 1, got {a.dim}")
    if a.sde == "vanderpol" and a.dim != 2:
        p.error("the Van der Pol oscillator has two state dimensions: use -dim 2")
    if a.sde in ("benes", "sine", "sqrt") and a.dim > 4:
        p.error(f"-sde {a.sde} is built for state dimensions up to 4")
    if not a.diffusion > 0:
        p.error(f"-q must be positive, got {a.diffusion}")
    if a.sigma < 0:
        p.error(f"-si must be non-negative, got {a.sigma}")
    if a.seed < 0:
        p.error(f"-s must be non-negative, got {a.seed}")
    T = time_grid_of(a.t0, a.t1, a.dt).shape[0]
    if not 1 <= a.num_observations <= T:
        p.error(f"-n must be between 1 and the {T} points of the time grid, got {a.num_observations}")
    return a


def make_sde(name, q, decay=0.5):
    """The reference's choice of prior per name (generate_data.py:105-118)."""
    import torch

    from . import sde as S
    q = torch.as_tensor(q, dtype=torch.float64)
    if name == "ou":
        return S.OrnsteinUhlenbeckSDE(decay=decay, q=q)
    if name == "dw":
        return S.DoubleWellSDE(q=q)
    if name == "benes":
        return S.BenesSDE(q=q)
    if name == "sine":
        return S.SineDiffusionSDE(q=q)
    if name == "sqrt":
        return S.SqrtDiffusionSDE(q=q)
    if name == "vanderpol":
        return S.VanderPolOscillatorSDE(a=2.0, tau=5.0, q=q)
    raise ValueError(f"SDE {name!r} is not supported")


def get_observations(sde, t0, t1, x0, dt, noise_std, num_observations, seed=0, device="cuda"):
    """(latent [N, d], observation_grid, observations, time_grid, test_grid, test_observations) -- generate_data.py:22-49."""
    import torch

    from .sde_utils import euler_maruyama
    rng = np.random.default_rng(seed)
    time_grid = time_grid_of(t0, t1, dt)
    x0 = torch.as_tensor(np.asarray(x0, dtype=np.float64).reshape(1, -1), device=device)
    latent = euler_maruyama(sde, x0, torch.as_tensor(time_grid, device=device), seed=seed)[0].cpu().numpy()

    def observe(n):
        grid = np.sort(rng.choice(time_grid, n, replace=False))
        idx = np.searchsorted(time_grid, grid)
        return grid, latent[idx] + rng.normal(scale=noise_std, size=(n, latent.shape[-1]))

    obs_grid, obs = observe(num_observations)
    test_grid, test_obs = observe(int(0.2 * num_observations))
    return latent, obs_grid, obs, time_grid, test_grid, test_obs


def main(argv=None):
    a = parse_args(argv)
    q = a.diffusion * np.eye(a.dim, dtype=np.float64)
    x0 = a.x0 * np.ones((1, a.dim), dtype=np.float64)
    sde = make_sde(a.sde, q, a.decay)
    latent, obs_grid, obs, time_grid, test_grid, test_obs = get_observations(sde, a.t0, a.t1, x0, a.dt, a.sigma, a.num_observations,
                                                                             seed=a.seed)
    output_path = str(a.seed) if a.output == "" else os.path.join(a.output, str(a.seed))
    if a.output:
        os.makedirs(a.output, exist_ok=True)
    np.savez(output_path, sde=a.sde, decay=a.decay, Q=q, x0=x0, sigma=a.sigma, latent_process=latent, observations=obs,
             observation_grid=obs_grid, time_grid=time_grid, test_observations=test_obs, test_grid=test_grid)
    print(f"Number of observations = {obs_grid.shape[0]}")
    print(f"Number of test-observations = {test_grid.shape[0]}")
    return output_path + ".npz"


if __name__ == "__main__":
    main()
