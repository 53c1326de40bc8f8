"""
Seeded draws from a factorised Gauss-Markov distribution (include/mfgm.h, `mfgm_packed_sample`).

With the natural-order block Cholesky factor  Lambda = L L^T  of a form-0 factorisation and  y = L^{-1} r  (what `Plan.factor` returns),
a draw is one backward substitution

    x = L^{-T} (y + eps),     eps[n, b, t, :] = normal_stream(S, B T, d, seed, stream)[n, b T + t, :]

Stream tags: 1 for posterior draws (`StateSpaceModel.sample(seed=...)`, the conditioning-point draw of `ConditionalProcess`), 2 for the
prior draw at the joint time points inside `ConditionalProcess`.  Lane-per-segment plans (d <= 8) run the native kernel; wide plans
(d > 8) take the fallback route: natural-layout L, G, y and `mfgm_bidiag_solve` (transposed) on y + eps, one sample at a time.  The
fallback is also the route the native kernel is checked against.
"""
import torch

from . import _lib
from ._lib import FULL, TRI, VEC
from .packed import _ptr, _stream

POSTERIOR_STREAM = 1
PRIOR_STREAM = 2


def sample_shape_tuple(sample_shape):
    """The reference's SampleShape (an int or a sequence of ints) as a tuple, and the number of samples it holds."""
    if isinstance(sample_shape, int):
        sample_shape = (sample_shape,)
    shape = tuple(int(v) for v in sample_shape)
    if any(v < 0 for v in shape):
        raise ValueError(f"sample_shape must not be negative, got {shape}")
    S = 1
    for v in shape:
        S *= v
    return shape, S


def check_seed(seed, stream):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    if not 0 <= int(stream) < 2 ** 32:
        raise ValueError("the stream tag is a 32-bit word")
    return seed, int(stream)


def _check_factor(plan, f):
    if f.get("form", 0) != 0:
        raise ValueError("sample: the factor is in inverse form (form 1); factorise with moments_only=False")
    if f.get("G") is None:
        raise ValueError("sample: the factor was taken with store_G=False (L_{t+1,t} is needed)")
    if f.get("y") is None:
        raise ValueError("sample: the factor has no forward substitution y = L^{-1} r (factorise with a right-hand side)")
    if plan.B * plan.T >= 2 ** 32:
        raise ValueError("sample: B T >= 2^32 (the stream's step counter is a 32-bit word)")


def native_sample(plan, f, n_samples, seed, stream=POSTERIOR_STREAM):
    """x [S, B, T, d] from the packed factor `f` by the HIP kernel (d <= 8)."""
    seed, stream = check_seed(seed, stream)
    S = int(n_samples)
    if S < 0:
        raise ValueError("sample: n_samples must not be negative")
    _check_factor(plan, f)
    if plan.wide:
        raise ValueError("sample: the native sampler covers lane-per-segment plans (d <= 8); use fallback_sample")
    x = torch.empty((S, plan.B, plan.T, plan.d), dtype=torch.float64, device=plan.device)
    if S == 0:
        return x
    scratch = torch.empty(max(int(plan.lib.mfgm_packed_sample_scratch_doubles(plan.h, S)), 1), dtype=torch.float64, device=plan.device)
    _lib.check(plan.lib.mfgm_packed_sample(plan.h, _ptr(f["L"]), _ptr(f["G"]), _ptr(f["y"]), S, seed, stream, _ptr(x), _ptr(scratch),
                                           _stream()), "mfgm_packed_sample")
    return x


def fallback_sample(plan, f, n_samples, seed, stream=POSTERIOR_STREAM):
    """The same draw through natural-layout L, G, y and mfgm_bidiag_solve (transposed) on y + eps, one sample at a time (any d <= 32)."""
    from .sde_utils import normal_stream
    seed, stream = check_seed(seed, stream)
    S = int(n_samples)
    if S < 0:
        raise ValueError("sample: n_samples must not be negative")
    _check_factor(plan, f)
    B, T, d = plan.B, plan.T, plan.d
    x = torch.empty((S, B, T, d), dtype=torch.float64, device=plan.device)
    if S == 0:
        return x
    Ld = plan.unpack(TRI, f["L"])
    Ls = plan.unpack(FULL, f["G"], T - 1) if T > 1 else torch.zeros((B, 1, d, d), dtype=torch.float64, device=plan.device)
    y = plan.unpack(VEC, f["y"])
    lib = plan.lib
    scratch = torch.empty(max(int(lib.mfgm_bidiag_scratch_doubles(B, T, d)), 1), dtype=torch.float64, device=plan.device)
    eps = normal_stream(S, B * T, d, seed=seed, stream=stream, device=plan.device).view(S, B, T, d)
    with torch.cuda.device(plan.device):
        for n in range(S):
            rhs = (y + eps[n]).contiguous()
            _lib.check(lib.mfgm_bidiag_solve(B, T, d, _ptr(Ld), _ptr(Ls), _ptr(rhs), _ptr(x[n]), 1, _ptr(scratch), _stream()),
                       "mfgm_bidiag_solve")
    return x


def sample(plan, f, n_samples, seed, stream=POSTERIOR_STREAM):
    """Native kernel for lane-per-segment plans, the fallback route for wide ones."""
    if plan.wide:
        return fallback_sample(plan, f, n_samples, seed, stream)
    return native_sample(plan, f, n_samples, seed, stream)
