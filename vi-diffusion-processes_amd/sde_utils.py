"""
Simulation of the SDE priors: `euler_maruyama` (markovflow/sde/sde_utils.py:36-96) on the HIP kernel of csrc/mfgm_sim.h, and
`normal_stream`, the counter-based normal stream it draws from (include/mfgm.h `mfgm_normal_fill`).

The drifts with a kernel are the drift methods of the classes in `NATIVE_DRIFTS` (kinds of mfgm_quad_drift); any other drift runs a torch
loop with the same noise, so the two routes agree path for path.
"""
import ctypes

import torch

from . import _lib
from . import sde as _sde
from .packed import _ptr, _stream

MAX_STATE_DIM = 8       # kSimD of csrc/mfgm_sim.h

# `type(sde).drift` -> kernel drift kind (include/mfgm.h, mfgm_quad_drift); a subclass that overrides `drift` is not in this table
NATIVE_DRIFTS = {
    _sde.VanderPolOscillatorSDE.drift: 10,
    _sde.MLPDrift.drift: 11,
    _sde.OrnsteinUhlenbeckSDE.drift: 12,
    _sde.DoubleWellSDE.drift: 12,
    _sde.BenesSDE.drift: 13,
    _sde.SineDiffusionSDE.drift: 14,
    _sde.SqrtDiffusionSDE.drift: 15,
}


def _theta(sde, kind):
    """The drift parameters as the kernel reads them, taken from the attributes the torch drift reads (so at call time: a prior that was
    learnt or assigned since is the one simulated), and the hidden width (kind 11)."""
    if kind == 10:
        return [sde.a, sde.tau], 0
    if kind == 11:
        W1, b1, W2, b2 = sde.weights
        return [float(v) for v in torch.cat([W1.reshape(-1), b1.reshape(-1), W2.reshape(-1), b2.reshape(-1)])], int(b1.numel())
    if kind == 12:
        return list(sde.drift_cubic()), 0
    return [sde.theta, 0.0], 0


def native_kind(sde):
    """The kernel drift kind that simulates `sde`, or None when its drift has no kernel (or exceeds the kernel's limits)."""
    kind = NATIVE_DRIFTS.get(getattr(type(sde), "drift", None))
    if kind is None or sde.state_dim > MAX_STATE_DIM:
        return None
    if kind == 10 and sde.state_dim != 2:
        return None
    if kind == 11 and len(_theta(sde, kind)[0]) > _lib.QUAD_NTHETA:
        return None
    return kind


def _check_seed(seed):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    return seed


def normal_stream(P, K, d, seed=0, stream=0, device="cuda"):
    """z [P, K, d]: normals of paths 0..P-1, steps 0..K-1 of the Philox4x32-10 / Box-Muller stream `stream` (0 = Euler-Maruyama
    increments), the contract stated in include/mfgm.h."""
    if min(P, K) < 0 or d < 1:
        raise ValueError(f"normal_stream: bad shape ({P}, {K}, {d})")
    if not 0 <= int(stream) < 2 ** 32:
        raise ValueError("normal_stream: the stream tag is a 32-bit word")
    out = torch.empty((P, K, d), dtype=torch.float64, device=device)
    if out.device.type != "cuda":
        raise ValueError("normal_stream: the stream is generated on the GPU")
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().mfgm_normal_fill(_check_seed(seed), int(stream), P, K, d, _ptr(out), _stream()), "mfgm_normal_fill")
    return out


def _chol_q(sde, d):
    q = torch.as_tensor(sde.q, dtype=torch.float64).detach().cpu().reshape(d, d)
    return torch.linalg.cholesky(q)


def _torch_route(sde, x0, tg, L, seed):
    """The reference's scan, one torch op at a time: drift(x, t) with t [B, 1] = t_{k-1}, noise from the stream above."""
    B, d = x0.shape
    N = tg.shape[0]
    dev = x0.device
    noise_dev = dev if dev.type == "cuda" else torch.device("cuda")
    z = normal_stream(B, max(N - 1, 0), d, seed=seed, device=noise_dev).to(dev)
    L = L.to(dev)
    t_prev = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), tg[:-1]])
    dts = tg - t_prev
    sqs = torch.sqrt(dts)
    X = torch.empty((B, N, d), dtype=torch.float64, device=dev)
    X[:, 0] = x0
    x = x0
    for k in range(N - 1):
        zk = z[:, k]
        Lz = zk[:, 0:1] * L[:, 0]
        for j in range(1, d):
            Lz = Lz + zk[:, j:j + 1] * L[:, j]
        t = t_prev[k].expand(B, 1)
        x = x + sde.drift(x, t) * dts[k] + sqs[k] * Lz
        X[:, k + 1] = x
    return X


def euler_maruyama(sde, x0, time_grid, *, seed=0, native=None):
    """Euler-Maruyama simulation of dx = f(x, t) dt + L dB, L = chol(q) (markovflow/sde/sde_utils.py:36-96, with its time alignment):
    t_{-1} = 0, dt_k = t_k - t_{k-1},

        X[:, 0] = x0,   X[:, k+1] = X[:, k] + f(X[:, k]) dt_k + sqrt(dt_k) L z[:, k]      (k = 0 .. N-2)

    (the reference's last scan step is dropped, so a grid starting at 0 repeats x0).  x0 [B, d], time_grid [N] non-decreasing with
    t_0 >= 0 -> X [B, N, d] float64 on x0's device.

    `seed` selects the counter-based normal stream (include/mfgm.h): the noise of path i at step k depends on (seed, i, k) only.  `native`:
    None takes the HIP kernel when the drift is one of NATIVE_DRIFTS within its limits and x0 is on the GPU, else the torch loop (same
    noise); True requires the kernel (ValueError otherwise); False forces the torch loop.  Both keywords are additions to the reference."""
    x0 = torch.as_tensor(x0, dtype=torch.float64)
    if x0.dim() != 2:
        raise ValueError(f"x0 must be [num_batch, state_dim], got shape {tuple(x0.shape)}")
    B, d = x0.shape
    if d != sde.state_dim:
        raise ValueError(f"x0 has state dimension {d}, the SDE {sde.state_dim}")
    if B < 1:
        raise ValueError("x0 holds no path")
    tg = torch.as_tensor(time_grid, dtype=torch.float64).to(x0.device).reshape(-1)
    if tg.numel() < 1:
        raise ValueError("empty time grid")
    tgh = tg.cpu()
    if not bool(torch.isfinite(tgh).all()):
        raise ValueError("the time grid is not finite")
    if float(tgh[0]) < 0.0:
        raise ValueError(f"the time grid starts at {float(tgh[0])} < 0 (the reference's first step is t_0 - 0)")
    if tgh.numel() > 1 and bool((tgh[1:] < tgh[:-1]).any()):
        raise ValueError("the time grid decreases")
    seed = _check_seed(seed)
    L = _chol_q(sde, d)
    kind = native_kind(sde)
    if native is True:
        if kind is None:
            raise ValueError(f"{type(sde).__name__}: no Euler-Maruyama kernel for this drift (kernels: {sorted(c.__qualname__ for c in NATIVE_DRIFTS)}, "
                             f"state_dim <= {MAX_STATE_DIM})")
        if x0.device.type != "cuda":
            raise ValueError("the Euler-Maruyama kernel needs x0 on the GPU")
    use_native = native is not False and kind is not None and x0.device.type == "cuda"
    if not use_native:
        return _torch_route(sde, x0, tg, L, seed)
    th, nh = _theta(sde, kind)
    prm = _lib.QuadDrift()
    prm.kind, prm.d, prm.nh = kind, d, nh
    for k, v in enumerate(th):
        prm.theta[k] = float(v)
    Lh = (ctypes.c_double * (d * d))(*[float(v) for v in L.reshape(-1)])
    x0c, tgc = x0.contiguous(), tg.contiguous()
    N = tgc.shape[0]
    X = torch.empty((B, N, d), dtype=torch.float64, device=x0.device)
    with torch.cuda.device(x0.device):
        _lib.check(_lib.load().mfgm_euler_maruyama(ctypes.byref(prm), B, N, _ptr(x0c), _ptr(tgc), Lh, seed, _ptr(X), _stream()),
                   "mfgm_euler_maruyama")
    return X
