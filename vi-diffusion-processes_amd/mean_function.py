"""
Host-side mirror of markovflow/mean_function.py: `MeanFunction`, `ZeroMeanFunction`, `LinearMeanFunction`, `ImpulseMeanFunction`,
`StepMeanFunction` (mean_function.py:27-413), the reference's names and signatures.

The two action classes are the deterministic response of the kernel's own dynamics dx = F x dt + u(t) dt + L dw to a control input:
impulses u(t) = sum_k u_k delta(t - t_k), or steps u(t) = u_k on (t_k, t_k+1].  With j = #{k : t_k < t} (searchsorted, left):
mu(t) = 0 for j = 0, otherwise with k = j - 1

    mu(t) = s_k + A(t - t_k) c_k,       c_k = A(t_k - t_k-1) c_k-1 + rhs_k,  c_-1 = 0,

impulse: s = 0, rhs = u;  step: a_k = -G^-1 u_k, a_-1 = 0, s_k = a_k, rhs_k = a_k-1 - a_k, where G generates the kernel's transitions,
A(dt) = expm(G dt) (`kernel.generator_matrix`: the feedback matrix, except under a Product, whose `feedback_matrix` keeps the
reference's Kronecker PRODUCT while its transitions follow the Kronecker sum).  An action is not seen at its own time, only after it.
The observed mean is H mu(t) with the kernel's emission row; the kernel's own state_mean does not enter (superposition: the SSM
offsets carry it).

Two routes.  Native (any tree `_terms()` expresses with state_dim <= 8, CUDA tensors): the coefficient recurrence is a segmented scan
in at most three launches and the evaluation one launch with the transition, mat-vec, shift and emission in registers
(csrc/mfgm_mean.h).  Torch (state_dim > 8, the LEG kernel, CPU tensors, VIDP_NATIVE_MEAN=0): the reference's
algorithm on existing pieces -- LowerTriangularBlockTriDiagonal(I, -A).solve on the device (the plain recurrence on the host),
searchsorted, gathers and transition_statistics_local.  The coefficients are cached on the instance, keyed by the kernel's current
terms (hyper-parameter values on the torch route) and the action tensors' stamps.
"""
import ctypes
import os

import torch

from . import _lib
from .stamps import Stamp


class MeanFunction:
    """mean_function.py:27-62.  __call__(time_points [..., N]) -> [..., N, obs_dim]."""

    depends_on_kernel = False

    def __call__(self, time_points):
        raise NotImplementedError

    def kernel_changed(self):
        """The kernel's hyper-parameters were assigned: drop what was derived from them (nothing here)."""


class ZeroMeanFunction(MeanFunction):
    """mean_function.py:65-87."""

    def __init__(self, obs_dim):
        self._obs_dim = int(obs_dim)

    def __call__(self, time_points):
        return torch.zeros(tuple(time_points.shape) + (self._obs_dim,), dtype=time_points.dtype, device=time_points.device)


class LinearMeanFunction(MeanFunction):
    """mean_function.py:90-114: m(t) = coefficient * t on every output."""

    def __init__(self, coefficient, obs_dim=1):
        self._coefficient = coefficient
        self._obs_dim = int(obs_dim)

    def __call__(self, time_points):
        return (self._coefficient * time_points[..., None]).expand(tuple(time_points.shape) + (self._obs_dim,))


def _freeze(x):
    """A nested structure of dicts / lists / tensors / numbers as a hashable, comparable value."""
    if isinstance(x, dict):
        return tuple((k, _freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_freeze(v) for v in x)
    if isinstance(x, torch.Tensor):
        return tuple(x.detach().reshape(-1).tolist())
    return x


class _ActionMeanFunction(MeanFunction):
    """What ImpulseMeanFunction and StepMeanFunction share: the checks, the two routes and the coefficient cache."""

    depends_on_kernel = True

    def __init__(self, action_times, state_perturbations, kernel):
        from .kernels import StationaryKernel
        if not isinstance(kernel, StationaryKernel):
            raise NotImplementedError(f"{type(self).__name__} needs a stationary kernel with state_transitions, got "
                                      f"{type(kernel).__name__} (a PiecewiseKernel has no single transition semigroup)")
        action_times = torch.as_tensor(action_times, dtype=torch.float64)
        state_perturbations = torch.as_tensor(state_perturbations, dtype=torch.float64)
        if state_perturbations.dim() < 2 or tuple(action_times.shape) != tuple(state_perturbations.shape[:-1]):
            raise ValueError(f"action_times {tuple(action_times.shape)} and state_perturbations {tuple(state_perturbations.shape)} must be "
                             "[..., K] and [..., K, state_dim]")
        if state_perturbations.shape[-1] != kernel.state_dim:
            raise ValueError(f"state_perturbations must have state_dim = {kernel.state_dim} entries per action, got "
                             f"{state_perturbations.shape[-1]}")
        if action_times.shape[-1] < 1:
            raise ValueError("at least one action is needed")
        if not bool(torch.isfinite(action_times).all()) or not bool((action_times[..., 1:] >= action_times[..., :-1]).all()):
            raise ValueError("action_times must be finite and non-decreasing along the last axis")
        self._kernel = kernel
        self._action_times, self._state_perturbations = action_times, state_perturbations
        self._batch_shape = tuple(action_times.shape[:-1])
        self._num_actions, self._state_dim = int(action_times.shape[-1]), int(kernel.state_dim)
        self._cache = {}

    # -- what the two classes differ in ---------------------------------------------------------------------------------------------------
    def _rhs_shift(self, u):
        """(rhs, shift) [B, K, d] of the perturbations u [B, K, d]; shift None for zero."""
        raise NotImplementedError

    # -- routes ---------------------------------------------------------------------------------------------------------------------------
    def _native(self, device):
        """The kernel's terms when the HIP route applies on this device, else None."""
        if device.type != "cuda" or self._state_dim > 8 or os.environ.get("VIDP_NATIVE_MEAN", "1") == "0":
            return None
        terms = self._kernel._terms()
        if terms is None or len(terms) > 8:
            return None
        return terms

    def kernel_changed(self):
        self._cache = {}

    def _coefficients(self, device):
        """dict(times [B, K], coef [B, K, d], shift [B, K, d] or None, terms) on the device, cached until the kernel's parameters or
        the action tensors move."""
        terms = self._native(device)
        key = _freeze(terms) if terms is not None else _freeze(self._kernel.hyperparameter_values())
        parts = (key, self._action_times, self._state_perturbations)
        c = self._cache.get(device)
        if c is not None and c["stamp"].matches(*parts):
            return c
        K, d = self._num_actions, self._state_dim
        times = self._action_times.to(device).reshape(-1, K).contiguous()
        u = self._state_perturbations.to(device).reshape(-1, K, d).contiguous()
        rhs, shift = self._rhs_shift(u)
        if terms is not None:
            coef = self._scan_native(terms, times, rhs.contiguous())
        else:
            coef = self._scan_torch(times, rhs)
        c = dict(stamp=Stamp(*parts), times=times, coef=coef, shift=None if shift is None else shift.contiguous(), terms=terms)
        self._cache[device] = c
        return c

    def _scan_native(self, terms, times, rhs, seg_len=0):
        lib = _lib.load()
        B, K, d = rhs.shape
        kt = self._kernel._terms_struct(terms)
        coef = torch.empty_like(rhs)
        ws = torch.empty(max(lib.mfgm_action_workspace_doubles(B, K, d, seg_len), 1), dtype=torch.float64, device=rhs.device)
        from .packed import _ptr, _stream
        with torch.cuda.device(rhs.device):
            _lib.check(lib.mfgm_action_coefficients(ctypes.byref(kt), B, K, seg_len, _ptr(times), _ptr(rhs), _ptr(coef), _ptr(ws),
                                                    _stream()), "mfgm_action_coefficients")
        return coef

    def _scan_torch(self, times, rhs):
        """The reference's block-bidiagonal solve [I; -A_k I] c = rhs (mean_function.py:195-223, 347-375)."""
        B, K, d = rhs.shape
        if K == 1:
            return rhs.clone()
        A = self._kernel.transition_statistics_local(times[:, 1:] - times[:, :-1])[0]
        if rhs.is_cuda and d <= 32:
            from .block_tri_diag import LowerTriangularBlockTriDiagonal
            eye = torch.eye(d, dtype=torch.float64, device=rhs.device).expand(B, K, d, d).contiguous()
            return LowerTriangularBlockTriDiagonal(eye, (-A).contiguous()).solve(rhs)
        coef = torch.empty_like(rhs)
        c = rhs[:, 0]
        coef[:, 0] = c
        for k in range(1, K):
            c = (A[:, k - 1] @ c[..., None])[..., 0] + rhs[:, k]
            coef[:, k] = c
        return coef

    # -- evaluation -----------------------------------------------------------------------------------------------------------------------
    def _flat_points(self, time_points):
        """time_points [..., N] -> ([B, N'] contiguous on its device, the shape to give back without the trailing d)."""
        tp = torch.as_tensor(time_points, dtype=torch.float64)
        if tp.dim() < 1:
            raise ValueError("time_points must be [..., N]")
        bs = self._batch_shape
        if bs == ():
            return tp.reshape(1, -1).contiguous(), tuple(tp.shape)
        shape = torch.broadcast_shapes(tuple(tp.shape[:-1]), bs) + (tp.shape[-1],)
        if tuple(shape[:-1]) != bs:
            raise ValueError(f"time_points {tuple(tp.shape)} do not broadcast to the actions' batch shape {bs}")
        return tp.expand(shape).reshape(-1, shape[-1]).contiguous(), tuple(shape)

    def _evaluate(self, time_points, want_state, want_f):
        tp, shape = self._flat_points(time_points)
        c = self._coefficients(tp.device)
        B, N = tp.shape
        K, d = self._num_actions, self._state_dim
        h = self._kernel._emission_row().to(torch.float64)
        state = f = None
        if c["terms"] is not None:
            lib = _lib.load()
            from .packed import _ptr, _stream
            kt = self._kernel._terms_struct(c["terms"])
            if want_state:
                state = torch.empty((B, N, d), dtype=torch.float64, device=tp.device)
            if want_f:
                f = torch.empty((B, N), dtype=torch.float64, device=tp.device)
            hrow = (ctypes.c_double * d)(*h.tolist())
            with torch.cuda.device(tp.device):
                _lib.check(lib.mfgm_action_mean(ctypes.byref(kt), B, K, N, _ptr(c["times"]), _ptr(c["coef"]), _ptr(c["shift"]), _ptr(tp),
                                                ctypes.cast(hrow, ctypes.c_void_p), _ptr(state), _ptr(f), _stream()), "mfgm_action_mean")
        else:
            state = self._evaluate_torch(c, tp)
            if want_f:
                f = state @ h.to(tp.device)
        return (None if state is None or not want_state else state.reshape(shape + (d,)),
                None if f is None else f.reshape(shape + (1,)))

    def _evaluate_torch(self, c, tp):
        """mean_function.py:225-258, 377-412: searchsorted, gathers, one transition per query point, a batched mat-vec."""
        times, coef, shift = c["times"], c["coef"], c["shift"]
        d = self._state_dim
        j = torch.searchsorted(times, tp, right=False)              # #{k : t_k < t}
        seen = j > 0
        k = (j - 1).clamp_min(0)
        dt = torch.where(seen, tp - torch.gather(times, 1, k), torch.zeros_like(tp))
        A = self._kernel.transition_statistics_local(dt)[0]
        kk = k[..., None].expand(tuple(k.shape) + (d,))
        mu = (A @ torch.gather(coef, 1, kk)[..., None])[..., 0]
        if shift is not None:
            mu = mu + torch.gather(shift, 1, kk)
        return torch.where(seen[..., None], mu, torch.zeros_like(mu))

    def state_mean(self, time_points):
        """mu(t) [..., N, state_dim]: the mean before the emission."""
        return self._evaluate(time_points, True, False)[0]

    def __call__(self, time_points):
        """H mu(t) [..., N, 1]."""
        return self._evaluate(time_points, False, True)[1]


class ImpulseMeanFunction(_ActionMeanFunction):
    """mean_function.py:117-258: kicks u_k at the times t_k."""

    def _rhs_shift(self, u):
        return u, None


def _step_levels(kernel, u):
    """a_k = -G^-1 u_k for u [..., d] (one solve against the [d, d] generator); ValueError naming the kernel when G is singular."""
    G = kernel.generator_matrix.to(u.device, torch.float64)
    try:
        a = -torch.linalg.solve(G, u.reshape(-1, u.shape[-1]).transpose(0, 1)).transpose(0, 1).reshape(u.shape)
    except RuntimeError as e:          # torch.linalg.LinAlgError: exactly singular
        a = None
        err = e
    if a is None or not bool(torch.isfinite(a).all()):
        raise ValueError(f"StepMeanFunction needs an invertible feedback matrix: that of {type(kernel).__name__} is singular (a Constant "
                         "factor has F = 0, and a constant drive then grows without bound)") from (err if a is None else None)
    return a


class StepMeanFunction(_ActionMeanFunction):
    """mean_function.py:261-412: a piecewise-constant control signal, u(t) = u_k on (t_k, t_k+1]."""

    def __init__(self, action_times, state_perturbations, kernel):
        super().__init__(action_times, state_perturbations, kernel)
        _step_levels(kernel, torch.zeros(1, kernel.state_dim, dtype=torch.float64))      # the invertibility check, once

    def _rhs_shift(self, u):
        a = _step_levels(self._kernel, u)
        rhs = -a
        rhs[:, 1:] += a[:, :-1]
        return rhs, a
