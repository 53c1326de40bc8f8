"""
Host-side mirror of the SDE kernels on the path (markovflow/kernels/matern.py: `Matern12`, `OrnsteinUhlenbeck`, `Matern32`,
`Matern52`; kernels/periodic.py `HarmonicOscillator`; kernels/constant.py `Constant`; kernels/sde_kernel.py: `StationaryKernel`,
`Sum`, `Product`; kernels/latent_exp_generated.py `LatentExponentiallyGenerated`; kernels/piecewise_stationary.py).

One closed-form route: a kernel class states its dynamics once, in `_parts` (A, Pinf and Q without jitter under the exact-Q rule of
DESIGN.md section 12, in torch, differentiable through the hyper-parameter leaves), `_emission_row`, `_terms` and `feedback_matrix`;
`StationaryKernel` derives the steady-state covariance, `transition_statistics_local`, `differentiable_ssm`, the emission model and
the torch construction beyond state_dim 8 from them.

`state_space_model(time_points)` for state_dim <= 8 is one HIP launch that evaluates the transitions, the process covariances and
their Cholesky factors directly in the packed layout: k_stationary_ssm for Matern / OU trees, the term kernel k_kernel_ssm
(mfgm_packed_kernel_ssm) for any other Sum / Product tree `_terms()` expresses, k_leg_ssm (mfgm_packed_leg_ssm)
for the learnable dynamics, which have no closed-form transition, and k_piecewise_ssm for change-point priors.
"""
import ctypes
import math
import os

import torch

from . import _lib, linalg
from .emission_model import EmissionModel
from .packed import Plan
from .state_space_model import StateSpaceModel, _flat
from .variational_cvi_sde import _ssm_from_packed


_FACTOR_DIM = {_lib.FACTOR_MATERN12: 1, _lib.FACTOR_MATERN32: 2, _lib.FACTOR_MATERN52: 3, _lib.FACTOR_CONSTANT: 1,
               _lib.FACTOR_HARMONIC: 2}
_NOT_PD = ("the process covariance Q of the kernel's state-space model is neither positive definite nor exactly zero "
           "(e.g. a Sum of a Matern and a HarmonicOscillator): set a jitter on the kernel")


# -- the tails every kernel class shares: transition statistics -> model ---------------------------------------------------------------
def _model_from_packed(plan, packed, batch_shape, not_pd=True):
    """StateSpaceModel of the packed (A, off, chol) one of the plan's SSM launches returned.  not_pd: a Q that is neither positive
    definite nor exactly zero raises the "set a jitter" ArithmeticError instead of the plan's own."""
    try:
        plan.check_info()
    except ArithmeticError as e:
        if not not_pd:
            raise
        raise ArithmeticError(_NOT_PD) from e
    ssm = _ssm_from_packed(plan, *packed)
    ssm.batch_shape = batch_shape
    return ssm


def _model_from_torch(A, Q, m, mu0, P0, plan, batch_shape):
    """StateSpaceModel of (A, Q) [B, T - 1, d, d] held in torch: cholesky_or_zero of Q and b = (I - A) m, with m [d] or [B, T - 1, d]
    the state means at the transitions' left ends; the first state is N(mu0 [d], P0 [d, d] or [B, d, d])."""
    B, d = A.shape[0], A.shape[-1]
    zero = (Q == 0).all(dim=-1).all(dim=-1)[..., None, None]
    chol = linalg.cholesky(torch.where(zero, torch.eye(d, dtype=Q.dtype, device=Q.device), Q))
    chol = torch.where(zero, torch.zeros_like(chol), chol)
    off = m - (A @ m[..., None])[..., 0]
    ssm = StateSpaceModel(mu0.expand(B, d).contiguous(), linalg.cholesky(P0).expand(B, d, d).contiguous(), A, off, chol, plan=plan)
    ssm.batch_shape = batch_shape
    return ssm


def _tape_model(A, Qterm, exact, Pinf0, m, mu0, jitter, plan):
    """tape.TapeSSM of one chain from differentiable A, Qterm = Pinf - A Pinf A^T [T - 1, d, d] (exactly zero when `exact`) and
    Pinf0 [d, d] of the first state: Q = Qterm + jitter, zero where that is exact, b = (I - A) m with m as in _model_from_torch."""
    from . import tape
    jit = jitter * torch.eye(A.shape[-1], dtype=torch.float64, device=A.device)
    Q = Qterm + jit
    b = m - (A @ m[..., None])[..., 0]
    cq = torch.zeros_like(Q) if (exact and jitter == 0.0) else tape.cholesky(0.5 * (Q + Q.transpose(-1, -2)))
    return tape.TapeSSM(mu0[None], tape.cholesky(Pinf0 + jit)[None], A[None], b[None], cq[None], plan=plan)


def _emission_model(H, time_points):
    """EmissionModel of the time-invariant H [output_dim, state_dim], tiled over the time points."""
    H = H.to(time_points.device)
    return EmissionModel(H.expand(tuple(time_points.shape) + tuple(H.shape)).contiguous(), constant_matrix=H)


class StationaryKernel:
    """kernels/sde_kernel.py:367-475.  A kernel class states its dynamics in _parts, _emission_row, _terms and feedback_matrix; every
    other member is derived from them here."""

    state_dim = None
    _matern_tree = True      # only Matern / OU leaves and Sums of them: what selects k_stationary_ssm in state_space_model

    def __init__(self, output_dim=1, jitter=0.0, state_mean=None):
        if output_dim != 1:
            raise ValueError("only output_dim == 1 kernels are on the hot path")
        self.output_dim = output_dim
        self.jitter = float(jitter)
        self._state_mean = state_mean

    @property
    def state_mean(self):
        if self._state_mean is None:
            return torch.zeros(self.state_dim, dtype=torch.float64)
        return torch.as_tensor(self._state_mean, dtype=torch.float64).reshape(self.state_dim)

    def set_state_mean(self, state_mean, trainable=False):
        self._state_mean = state_mean

    # -- the primitives: the Matern / OU leaf, whose subclasses give (order, lam, var) ---------------------------------------------------
    def _components(self):
        """[(order, lam, var)] of the Matern / OU blocks of this kernel, in state order."""
        raise NotImplementedError

    def _components_t(self, leaves):
        """[(order, lam, var)] with lam / var torch expressions of the leaves (the differentiable twin of _components)."""
        raise NotImplementedError

    def hyperparameter_leaves(self, device="cpu"):
        """{name: 0-dim tensor with requires_grad} of this kernel's trainable hyper-parameters (a list of such dicts for a Sum): the
        leaves of a torch graph (the reference differentiates classic_elbo through the kernel's tf.Variables with a GradientTape,
        tests/integration/models/test_variational_cvi.py:93-110)."""
        raise NotImplementedError

    def _parts(self, dt, leaves=None):
        """(A [..., d, d], Pinf [d, d], Qterm [..., d, d], exact) at the time gaps dt [...]: Qterm = Pinf - A Pinf A^T without jitter
        (exactly zero when `exact`).  leaves: hyperparameter_leaves() to differentiate through, or None for the current values.
        Here the formulas of k_stationary_ssm: A = e^{-lam dt} (I + N dt + N^2 dt^2 / 2)."""
        comps = self._components() if leaves is None else self._components_t(leaves)
        (order, lam, var), = comps
        lam = torch.as_tensor(lam, dtype=torch.float64, device=dt.device)
        var = torch.as_tensor(var, dtype=torch.float64, device=dt.device)
        t = dt[..., None, None]
        ex = torch.exp(-lam * t)
        eye = torch.eye(order, dtype=torch.float64, device=dt.device)
        one, zero = torch.ones_like(lam), torch.zeros_like(lam)
        if order == 1:
            A, P = ex * eye, var.reshape(1, 1)
        elif order == 2:
            N = torch.stack([torch.stack([lam, one]), torch.stack([-lam ** 2, -lam])])
            A = ex * (eye + N * t)
            P = var * torch.stack([torch.stack([one, zero]), torch.stack([zero, lam ** 2])])
        else:
            N = torch.stack([torch.stack([lam, one, zero]), torch.stack([zero, lam, one]),
                             torch.stack([-lam ** 3, -3.0 * lam ** 2, -2.0 * lam])])
            A = ex * (eye + N * t + (N @ N) * (0.5 * t * t))
            l23 = lam ** 2 / 3.0
            P = var * torch.stack([torch.stack([one, zero, -l23]), torch.stack([zero, l23, zero]), torch.stack([-l23, zero, lam ** 4])])
        return A, P, P - A @ P @ A.transpose(-1, -2), False

    def _emission_row(self):
        """H of this kernel as a [state_dim] vector."""
        h = torch.zeros(self.state_dim, dtype=torch.float64)
        h[0] = 1.0
        return h

    def _terms(self):
        """This kernel as mfgm_kernel_terms rows: [[(kind, rate, var), ...] per term], or None where the struct cannot express it."""
        (order, lam, var), = self._components()
        return [[(order, float(lam), float(var))]]

    def _terms_t(self, leaves):
        """_terms() with rate and var as torch expressions of hyperparameter_leaves() (its differentiable twin): what carries the
        device's score with respect to (rate, var) (mfgm_packed_kernel_score) back to the leaves."""
        (order, lam, var), = self._components_t(leaves)
        return [[(order, lam, var)]]

    # the names of the positive scalar hyper-parameters, in the order of hyperparameter_leaves()
    _hyper_names = ()

    def hyperparameter_values(self):
        """The current hyper-parameters as floats, in the structure of hyperparameter_leaves() (a dict, or a list of dicts for the
        children of a Sum / Product): the inverse of assign_hyperparameters."""
        return {n: getattr(self, n) for n in self._hyper_names}

    def assign_hyperparameters(self, values):
        """Write hyper-parameters (the structure of hyperparameter_leaves(); floats or 0-dim tensors) back into the kernel, under the
        constructors' validation: a non-positive lengthscale, variance, period, decay or diffusion raises ValueError."""
        if set(values) != set(self._hyper_names):
            raise ValueError(f"{type(self).__name__} takes the hyper-parameters {self._hyper_names}, got {tuple(values)}")
        vals = {n: float(values[n]) for n in self._hyper_names}
        for n, v in vals.items():
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError(f"{n} must be positive, got {v}")
        for n, v in vals.items():
            setattr(self, n, v)

    @property
    def feedback_matrix(self):
        (order, lam, _), = self._components()
        if order == 1:
            return torch.tensor([[-lam]], dtype=torch.float64)
        if order == 2:
            return torch.tensor([[0.0, 1.0], [-lam ** 2, -2.0 * lam]], dtype=torch.float64)
        return torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-lam ** 3, -3.0 * lam ** 2, -3.0 * lam]], dtype=torch.float64)

    @property
    def generator_matrix(self):
        """G with A(dt) = expm(G dt): feedback_matrix, except under a Product, whose feedback_matrix is the reference's (x) F_i while
        its transitions are generated by the Kronecker sum.  What the step mean function solves against (mean_function.py)."""
        return self.feedback_matrix

    # -- the device structs ---------------------------------------------------------------------------------------------------------------
    def _spec(self):
        comps = self._components()
        if len(comps) > 8 or self.state_dim > 8:
            raise ValueError("the HIP path supports up to 8 components and state_dim <= 8")
        spec = _lib.KernelSpec()
        spec.ncomp = len(comps)
        off = 0
        for i, (order, lam, var) in enumerate(comps):
            spec.order[i], spec.offset[i], spec.lam[i], spec.var[i] = order, off, lam, var
            off += order
        m = self.state_mean
        for i in range(self.state_dim):
            spec.mean[i] = float(m[i])
        spec.jitter = self.jitter
        return spec

    def _terms_struct(self, terms=None):
        """mfgm_kernel_terms of this kernel (any tree _terms() expresses, Matern-only ones included)."""
        terms = self._terms() if terms is None else terms
        if terms is None or len(terms) > 8 or self.state_dim > 8:
            raise ValueError("the term kernel takes up to 8 terms of up to 3 primitive factors and state_dim <= 8")
        kt = _lib.KernelTerms()
        kt.nterm = len(terms)
        off = 0
        for c, factors in enumerate(terms):
            kt.nfactor[c], kt.offset[c] = len(factors), off
            n = 1
            for f, (kind, rate, var) in enumerate(factors):
                kt.kind[c][f], kt.rate[c][f], kt.var[c][f] = kind, rate, var
                n *= _FACTOR_DIM[kind]
            off += n
        m = self.state_mean
        for i in range(self.state_dim):
            kt.mean[i] = float(m[i])
        kt.jitter = self.jitter
        return kt

    # -- derived from the primitives ------------------------------------------------------------------------------------------------------
    @property
    def steady_state_covariance(self):
        return self._parts(torch.zeros(1, dtype=torch.float64))[1].detach()

    def state_space_model(self, time_points, plan=None):
        """SDEKernel.state_space_model (sde_kernel.py:153-171): prior SSM at the given (sorted) time points [..., T].  state_dim <= 8:
        one launch, k_stationary_ssm for a Matern tree and k_kernel_ssm for any other tree _terms() expresses; otherwise the torch
        closed forms (_state_space_model_wide)."""
        t, bs = _flat(time_points, 1)
        B, T = t.shape
        if plan is None:
            plan = Plan(B, T, self.state_dim, device=t.device)
        dts = (t[:, 1:] - t[:, :-1]).contiguous()
        if self._matern_tree:
            if self.state_dim > 8:
                return self._state_space_model_wide(dts, bs, plan)
            return _model_from_packed(plan, plan.stationary_ssm(self._spec(), dts), bs, not_pd=False)
        terms = self._terms() if self.state_dim <= 8 else None
        if terms is None or len(terms) > 8:
            try:
                return self._state_space_model_wide(dts, bs, plan)
            except ArithmeticError as e:
                raise ArithmeticError(_NOT_PD) from e
        return _model_from_packed(plan, plan.kernel_ssm(self._terms_struct(terms), dts), bs)

    def _state_space_model_wide(self, dts, bs, plan):
        """
        state_dim > 8 (e.g. the reference's Sum of ten Matern-5/2, d = 30) or a tree the term struct cannot express: the fused kernels
        are specialised for d <= 8, so this one-off model construction uses the per-element closed forms in torch (Q under the exact-Q
        rule + jitter, cholesky_or_zero, b = (I - A) m); the sweeps that follow run in the wide HIP kernels.
        """
        A, Q = self.transition_statistics_local(dts)
        m = self.state_mean.to(dts.device)
        return _model_from_torch(A, Q, m, m, self.initial_covariance_matrix().to(dts.device), plan, bs)

    def transition_statistics(self, transition_times, time_deltas):
        """(A_k, Q_k) (sde_kernel.py:421-446), natural tensors."""
        td, bs = _flat(time_deltas, 1)
        B, N = td.shape
        t = torch.cat([torch.zeros((B, 1), dtype=td.dtype, device=td.device), torch.cumsum(td, dim=1)], dim=1)
        ssm = self.state_space_model(t)
        A = ssm.state_transitions
        c = ssm.cholesky_process_covariances
        return A.reshape(bs + tuple(A.shape[1:])), (c @ c.transpose(-1, -2)).reshape(bs + tuple(c.shape[1:]))

    def state_transitions(self, transition_times, time_deltas):
        return self.transition_statistics(transition_times, time_deltas)[0]

    def transition_statistics_local(self, time_deltas):
        """
        (A, Q) for arbitrary, unordered time gaps (any shape [...]) as per-element closed forms in torch under the exact-Q rule
        (DESIGN.md section 12): used by the conditionals (prediction between conditioning points, conditionals.py:207-256), which are
        embarrassingly parallel over query points.  Same formulas as k_stationary_ssm and k_kernel_ssm.
        """
        A, _, Qterm, _ = self._parts(time_deltas)
        return A, Qterm + self.jitter * torch.eye(self.state_dim, dtype=A.dtype, device=A.device)

    def differentiable_ssm(self, time_points, leaves=None, plan=None):
        """(tape.TapeSSM, leaves): the prior state-space model at the sorted time points [T] (one chain) as a differentiable function of
        the hyper-parameter leaves -- _parts in torch, d <= 8; everything sequential in time downstream (marginals, log-determinants)
        goes through vidp_amd.tape, i.e. the HIP sweeps with exact backward passes."""
        t = time_points.reshape(-1)
        if leaves is None:
            leaves = self.hyperparameter_leaves(t.device)
        A, Pinf, Qterm, exact = self._parts(t[1:] - t[:-1], leaves)
        m = self.state_mean.to(t.device)
        return _tape_model(A, Qterm, exact, Pinf, m, m, self.jitter, plan), leaves

    def initial_mean(self, batch_shape=()):
        return self.state_mean.expand(tuple(batch_shape) + (self.state_dim,))

    def initial_covariance_matrix(self):
        """Pinf + jitter (sde_kernel.py:402-419)."""
        return self.steady_state_covariance + self.jitter * torch.eye(self.state_dim, dtype=torch.float64)

    # -- the time-aware forms the models call (SDEKernel.initial_covariance / transition_statistics take the time of the state or of the
    #    transition's left end, sde_kernel.py:113-151): a stationary kernel ignores the times --------------------------------------------
    def initial_covariance(self, initial_time_point=None):
        return self.initial_covariance_matrix()

    def transition_statistics_at(self, transition_times, time_deltas):
        """(A, Q) of the transitions that start at transition_times and last time_deltas (any shape, unordered)."""
        return self.transition_statistics_local(time_deltas)

    def generate_emission_model(self, time_points):
        """H = _emission_row(), tiled over the time points (sde_kernel.py:173-211, 670-687)."""
        return _emission_model(self._emission_row()[None], time_points)


def _check(lengthscale, variance):
    if lengthscale <= 0.0 or variance <= 0.0:
        raise ValueError("lengthscale and variance must be positive")     # matern.py `_check_lengthscale_and_variance`


class Matern12(StationaryKernel):
    """matern.py:27-127."""
    state_dim = 1
    _hyper_names = ("lengthscale", "variance")

    def __init__(self, lengthscale, variance, output_dim=1, jitter=0.0):
        super().__init__(output_dim, jitter)
        _check(lengthscale, variance)
        self.lengthscale, self.variance = float(lengthscale), float(variance)

    def _components(self):
        return [(1, 1.0 / self.lengthscale, self.variance)]

    def hyperparameter_leaves(self, device="cpu"):
        mk = lambda v: torch.tensor(float(v), dtype=torch.float64, device=device, requires_grad=True)
        return {"lengthscale": mk(self.lengthscale), "variance": mk(self.variance)}

    def _components_t(self, leaves):
        return [(1, 1.0 / leaves["lengthscale"], leaves["variance"])]


class OrnsteinUhlenbeck(StationaryKernel):
    """matern.py:130-234: decay lambda, diffusion q, Pinf = q / (2 lambda)."""
    state_dim = 1
    _hyper_names = ("decay", "diffusion")

    def __init__(self, decay, diffusion, output_dim=1, jitter=0.0):
        super().__init__(output_dim, jitter)
        _check(decay, diffusion)
        self.decay, self.diffusion = float(decay), float(diffusion)

    def _components(self):
        return [(1, self.decay, self.diffusion / (2.0 * self.decay))]

    def hyperparameter_leaves(self, device="cpu"):
        mk = lambda v: torch.tensor(float(v), dtype=torch.float64, device=device, requires_grad=True)
        return {"decay": mk(self.decay), "diffusion": mk(self.diffusion)}

    def _components_t(self, leaves):
        return [(1, leaves["decay"], leaves["diffusion"] / (2.0 * leaves["decay"]))]


class Matern32(StationaryKernel):
    """matern.py:237-373."""
    state_dim = 2
    _hyper_names = ("lengthscale", "variance")

    def __init__(self, lengthscale, variance, output_dim=1, jitter=0.0):
        super().__init__(output_dim, jitter)
        _check(lengthscale, variance)
        self.lengthscale, self.variance = float(lengthscale), float(variance)

    def _components(self):
        return [(2, math.sqrt(3.0) / self.lengthscale, self.variance)]

    def hyperparameter_leaves(self, device="cpu"):
        mk = lambda v: torch.tensor(float(v), dtype=torch.float64, device=device, requires_grad=True)
        return {"lengthscale": mk(self.lengthscale), "variance": mk(self.variance)}

    def _components_t(self, leaves):
        return [(2, math.sqrt(3.0) / leaves["lengthscale"], leaves["variance"])]


class Matern52(StationaryKernel):
    """matern.py:376-520."""
    state_dim = 3
    _hyper_names = ("lengthscale", "variance")

    def __init__(self, lengthscale, variance, output_dim=1, jitter=0.0):
        super().__init__(output_dim, jitter)
        _check(lengthscale, variance)
        self.lengthscale, self.variance = float(lengthscale), float(variance)

    def _components(self):
        return [(3, math.sqrt(5.0) / self.lengthscale, self.variance)]

    def hyperparameter_leaves(self, device="cpu"):
        mk = lambda v: torch.tensor(float(v), dtype=torch.float64, device=device, requires_grad=True)
        return {"lengthscale": mk(self.lengthscale), "variance": mk(self.variance)}

    def _components_t(self, leaves):
        return [(3, math.sqrt(5.0) / leaves["lengthscale"], leaves["variance"])]


def _assign_children(kernels, values):
    """assign_hyperparameters of a Sum / Product: one entry of `values` per child; nothing is written unless every child accepts."""
    values = list(values)
    if len(values) != len(kernels):
        raise ValueError(f"expected hyper-parameters for {len(kernels)} child kernels, got {len(values)}")
    before = [k.hyperparameter_values() for k in kernels]
    try:
        for k, v in zip(kernels, values):
            k.assign_hyperparameters(v)
    except Exception:
        for k, v in zip(kernels, before):
            k.assign_hyperparameters(v)
        raise


class Sum(StationaryKernel):
    """sde_kernel.py:540-687 (ConcatKernel / Sum of stationary kernels): block-diagonal state, summed emissions."""

    def __init__(self, kernels, jitter=0.0):
        super().__init__(1, jitter)
        self.kernels = list(kernels)
        self.state_dim = sum(k.state_dim for k in self.kernels)

    @property
    def state_mean(self):
        return torch.cat([k.state_mean for k in self.kernels])

    def _components(self):
        out = []
        for k in self.kernels:
            out.extend(k._components())
        return out

    def hyperparameter_leaves(self, device="cpu"):
        return [k.hyperparameter_leaves(device) for k in self.kernels]

    @property
    def _matern_tree(self):
        return all(k._matern_tree for k in self.kernels)

    def _parts(self, dt, leaves=None):
        lv = [None] * len(self.kernels) if leaves is None else leaves
        parts = [k._parts(dt, l) for k, l in zip(self.kernels, lv)]
        return (_block_diag_b([p[0] for p in parts]), _block_diag_b([p[1] for p in parts]), _block_diag_b([p[2] for p in parts]),
                all(p[3] for p in parts))

    def _emission_row(self):
        return torch.cat([k._emission_row() for k in self.kernels])

    def _terms(self):
        out = []
        for k in self.kernels:
            t = k._terms()
            if t is None:
                return None
            out.extend(t)
        return out

    def _terms_t(self, leaves):
        out = []
        for k, lv in zip(self.kernels, leaves):
            t = k._terms_t(lv)
            if t is None:
                return None
            out.extend(t)
        return out

    def hyperparameter_values(self):
        return [k.hyperparameter_values() for k in self.kernels]

    def assign_hyperparameters(self, values):
        _assign_children(self.kernels, values)

    @property
    def feedback_matrix(self):
        return torch.block_diag(*[k.feedback_matrix for k in self.kernels])

    @property
    def generator_matrix(self):
        return torch.block_diag(*[k.generator_matrix for k in self.kernels])

    def state_space_model(self, time_points, plan=None):
        # each component kernel adds its own jitter to its Q block; Sum adds its own on top (sde_kernel.py:640-656).  (The torch build
        # of a Matern tree beyond state_dim 8 has always used the Sum's jitter alone.)
        if any(k.jitter != 0.0 for k in self.kernels) and not (self._matern_tree and self.state_dim > 8):
            raise ValueError("per-component jitter inside Sum is not supported on the HIP path; set it on the Sum")
        return super().state_space_model(time_points, plan)


def _kron(X, Y):
    """Kronecker product of the trailing square matrices, batch dimensions broadcast."""
    a, b = X.shape[-1], Y.shape[-1]
    out = X[..., :, None, :, None] * Y[..., None, :, None, :]
    return out.reshape(tuple(out.shape[:-4]) + (a * b, a * b))


def _block_diag_b(mats):
    """Block diagonal of [..., k, k] matrices, batch dimensions broadcast."""
    batch = torch.broadcast_shapes(*[m.shape[:-2] for m in mats])
    n = sum(m.shape[-1] for m in mats)
    out = torch.zeros(batch + (n, n), dtype=mats[0].dtype, device=mats[0].device)
    o = 0
    for m in mats:
        k = m.shape[-1]
        out[..., o:o + k, o:o + k] = m
        o += k
    return out


class HarmonicOscillator(StationaryKernel):
    """periodic.py:27-203: k(tau) = variance cos(2 pi tau / period); lambda = 2 pi / period, A = [[cos, -sin], [sin, cos]](lambda dt),
    Pinf = variance I, H = [1, 0], Q = 0 (+ jitter)."""
    state_dim = 2
    _matern_tree = False
    _hyper_names = ("variance", "period")

    def __init__(self, variance, period, output_dim=1, jitter=0.0):
        super().__init__(output_dim, jitter)
        if variance <= 0.0:
            raise ValueError("variance must be positive.")
        if period <= 0.0:
            raise ValueError("period must be positive.")
        self.variance, self.period = float(variance), float(period)

    @property
    def feedback_matrix(self):
        lam = 2.0 * math.pi / self.period
        return torch.tensor([[0.0, -lam], [lam, 0.0]], dtype=torch.float64)

    def hyperparameter_leaves(self, device="cpu"):
        mk = lambda v: torch.tensor(float(v), dtype=torch.float64, device=device, requires_grad=True)
        return {"variance": mk(self.variance), "period": mk(self.period)}

    def _parts(self, dt, leaves=None):
        var = torch.as_tensor(self.variance if leaves is None else leaves["variance"], dtype=torch.float64, device=dt.device)
        period = torch.as_tensor(self.period if leaves is None else leaves["period"], dtype=torch.float64, device=dt.device)
        x = (2.0 * math.pi / period) * dt[..., None, None]
        c, s = torch.cos(x), torch.sin(x)
        A = torch.cat([torch.cat([c, -s], dim=-1), torch.cat([s, c], dim=-1)], dim=-2)
        P = var * torch.eye(2, dtype=torch.float64, device=dt.device)
        return A, P, torch.zeros_like(A), True

    def _terms(self):
        return [[(_lib.FACTOR_HARMONIC, 2.0 * math.pi / self.period, self.variance)]]

    def _terms_t(self, leaves):
        return [[(_lib.FACTOR_HARMONIC, 2.0 * math.pi / leaves["period"], leaves["variance"])]]


class Constant(StationaryKernel):
    """constant.py:28-153: k(tau) = variance; A = [[1]], Pinf = [[variance]], H = [1], Q = 0 (+ jitter).  feedback_matrix is zero, as in
    the reference code (its docstring says [[1]])."""
    state_dim = 1
    _matern_tree = False
    _hyper_names = ("variance",)

    def __init__(self, variance, output_dim=1, jitter=0.0):
        super().__init__(output_dim, jitter)
        if variance <= 0:
            raise ValueError("variance must be positive.")
        self.variance = float(variance)

    @property
    def feedback_matrix(self):
        return torch.zeros((1, 1), dtype=torch.float64)

    def hyperparameter_leaves(self, device="cpu"):
        return {"variance": torch.tensor(self.variance, dtype=torch.float64, device=device, requires_grad=True)}

    def _parts(self, dt, leaves=None):
        var = torch.as_tensor(self.variance if leaves is None else leaves["variance"], dtype=torch.float64, device=dt.device)
        A = torch.ones(tuple(dt.shape) + (1, 1), dtype=torch.float64, device=dt.device)
        return A, var.reshape(1, 1), torch.zeros_like(A), True

    def _terms(self):
        return [[(_lib.FACTOR_CONSTANT, 0.0, self.variance)]]

    def _terms_t(self, leaves):
        return [[(_lib.FACTOR_CONSTANT, torch.zeros((), dtype=torch.float64, device=leaves["variance"].device), leaves["variance"])]]


class LatentExponentiallyGenerated(StationaryKernel):
    """kernels/latent_exp_generated.py:28-142, the LEG-GP kernel of Loper et al. (2020): dx = -1/2 G x dt + N dw with
    G = N N^T + R - R^T for arbitrary N (noise mixing) and R (rotation inducing) [d, d], so feedback_matrix F = -G / 2,
    steady_state_covariance = I, A(dt) = expm(F dt) and Q(dt) = I - A A^T.  The only kernel of the family whose dynamics are free
    parameters, and the only one without a closed-form transition.

    Emission: the reference sets output_dim = state_dim with every emission row e_1.  This package is single-output, so here
    output_dim = 1 and the emission row is e_1 by default, which fixes k(0) = 1; `emission` [d] supplies the LEG paper's B instead,
    k(tau) = B expm(F |tau|) B^T.  The emission is not trainable.

    state_dim <= 8 on the device: state_space_model is one launch of mfgm_packed_leg_ssm (scaling-and-squaring Taylor exponential, Q,
    chol Q and the offsets of every transition) and transition_statistics_local one of mfgm_leg_transitions;
    for state_dim > 8 or CPU tensors torch.linalg.matrix_exp (and, on the device, the wide sweeps).  _state_space_model_wide calls
    transition_statistics_local, so on the device with state_dim <= 8 it too takes the HIP transitions;
    StationaryKernel.transition_statistics_local is the torch route at any size.  Hyper-parameter gradients go through matrix_exp's
    backward and the tape.  Inside Sum / Product / PiecewiseKernel a LEG child takes the torch routes (_terms() is None)."""

    _matern_tree = False

    def __init__(self, N, R, jitter=0.0, emission=None):
        N = torch.as_tensor(N, dtype=torch.float64).detach().cpu()
        R = torch.as_tensor(R, dtype=torch.float64).detach().cpu()
        if N.dim() != 2 or N.shape[0] != N.shape[1] or N.shape[0] < 1 or tuple(R.shape) != tuple(N.shape):
            raise ValueError(f"N and R must be square matrices of one shape, got {tuple(N.shape)} and {tuple(R.shape)}")
        super().__init__(1, jitter)
        self.N, self.R = N.clone(), R.clone()
        self.state_dim = int(N.shape[0])
        if emission is not None:
            emission = torch.as_tensor(emission, dtype=torch.float64).detach().cpu().reshape(-1).clone()
            if emission.numel() != self.state_dim:
                raise ValueError(f"emission must have {self.state_dim} entries, got {emission.numel()}")
        self.emission = emission

    @staticmethod
    def _feedback(N, R):
        return -0.5 * (N @ N.transpose(-1, -2) + R - R.transpose(-1, -2))

    @property
    def feedback_matrix(self):
        return self._feedback(self.N, self.R)

    def hyperparameter_leaves(self, device="cpu"):
        mk = lambda v: v.clone().to(device).requires_grad_(True)
        return {"N": mk(self.N), "R": mk(self.R)}

    def _parts(self, dt, leaves=None):
        F = self.feedback_matrix.to(dt.device) if leaves is None else self._feedback(leaves["N"], leaves["R"])
        A = torch.linalg.matrix_exp(F * dt[..., None, None])
        eye = torch.eye(self.state_dim, dtype=torch.float64, device=dt.device)
        return A, eye, eye - A @ A.transpose(-1, -2), False

    def _emission_row(self):
        if self.emission is not None:
            return self.emission.clone()
        return super()._emission_row()

    def _terms(self):
        return None

    def _terms_t(self, leaves):
        return None

    def hyperparameter_values(self):
        """{"N", "R"}: copies of the two matrices (CPU fp64 tensors)."""
        return {"N": self.N.clone(), "R": self.R.clone()}

    def assign_hyperparameters(self, values):
        """N and R as [d, d] tensors (any values: the dynamics are unconstrained)."""
        if set(values) != {"N", "R"}:
            raise ValueError(f"LatentExponentiallyGenerated takes the hyper-parameters ('N', 'R'), got {tuple(values)}")
        N = torch.as_tensor(values["N"], dtype=torch.float64).detach().cpu()
        R = torch.as_tensor(values["R"], dtype=torch.float64).detach().cpu()
        d = self.state_dim
        if tuple(N.shape) != (d, d) or tuple(R.shape) != (d, d):
            raise ValueError(f"N and R must be [{d}, {d}], got {tuple(N.shape)} and {tuple(R.shape)}")
        if not (bool(torch.isfinite(N).all()) and bool(torch.isfinite(R).all())):
            raise ValueError("N and R must be finite")
        self.N, self.R = N.clone(), R.clone()

    def _spec(self):
        """mfgm_leg_spec of this kernel: F formed here, in fp64."""
        d = self.state_dim
        if d > 8:
            raise ValueError("the LEG kernels take state_dim <= 8")
        spec = _lib.LegSpec()
        spec.d = d
        F, m = self.feedback_matrix.reshape(-1).tolist(), self.state_mean.tolist()
        for e in range(d * d):
            spec.F[e] = F[e]
        for i in range(d):
            spec.mean[i] = m[i]
        spec.jitter = self.jitter
        return spec

    def state_space_model(self, time_points, plan=None):
        t, bs = _flat(time_points, 1)
        if self.state_dim > 8 or not t.is_cuda:
            return super().state_space_model(time_points, plan)
        B, T = t.shape
        if plan is None:
            plan = Plan(B, T, self.state_dim, device=t.device)
        return _model_from_packed(plan, plan.leg_ssm(self._spec(), (t[:, 1:] - t[:, :-1]).contiguous()), bs)

    def transition_statistics_local(self, time_deltas):
        """(A, Q) for arbitrary, unordered time gaps (any shape): one launch of mfgm_leg_transitions on the device for state_dim <= 8,
        torch.linalg.matrix_exp otherwise."""
        if self.state_dim > 8 or not time_deltas.is_cuda:
            return super().transition_statistics_local(time_deltas)
        from .packed import _ptr, _stream
        d = self.state_dim
        td = time_deltas.detach().to(torch.float64).contiguous()
        A = torch.empty(tuple(td.shape) + (d, d), dtype=torch.float64, device=td.device)
        Q = torch.empty_like(A)
        if td.numel():
            spec = self._spec()
            with torch.cuda.device(td.device):
                _lib.check(_lib.load().mfgm_leg_transitions(ctypes.byref(spec), td.numel(), _ptr(td), _ptr(A), _ptr(Q), _stream()),
                           "mfgm_leg_transitions")
        return A, Q


class Product(StationaryKernel):
    """sde_kernel.py:691-826: A = (x) A_i, Pinf = (x) Pinf_i, H = (x) H_i, state_dim = prod d_i.  Only the Product's own jitter is used
    (the children's is ignored, as in the reference, whose Product inherits transition_statistics and initial_covariance).

    Q follows the exact-Q rule: with M_i = A_i Pinf_i A_i^T (M_i = Pinf_i exactly for Constant and
    HarmonicOscillator, and for trees of them), Q = (x) Pinf_i - (x) M_i, rewritten as (Pinf_g - M_g) (x) (x)_{i != g} Pinf_i when g is
    the only child with M_g != Pinf_g, and exactly 0 when there is none."""

    _matern_tree = False

    def __init__(self, kernels, jitter=0.0):
        kernels = list(kernels)
        assert kernels, "There must be at least one child kernel."
        if not all(isinstance(k, StationaryKernel) for k in kernels):
            raise TypeError("can only combine Kernel instances")
        assert len(set(k.output_dim for k in kernels)) == 1, "All kernels must have the same output dimension"
        self.kernels = kernels
        self.state_dim = int(math.prod(k.state_dim for k in kernels))
        super().__init__(kernels[0].output_dim, jitter)

    @property
    def feedback_matrix(self):
        """(x) F_i, as the reference returns it.  NOT the generator of A = (x) expm(F_i dt): that is the Kronecker SUM
        F_1 (+) F_2 = F_1 (x) I + I (x) F_2.  Nothing in the package reads it."""
        F = self.kernels[0].feedback_matrix
        for k in self.kernels[1:]:
            F = _kron(F, k.feedback_matrix)
        return F

    @property
    def generator_matrix(self):
        """The Kronecker sum G_1 (+) G_2 (+) ...: A = (x) expm(G_i dt) = expm(((+) G_i) dt)."""
        G = self.kernels[0].generator_matrix
        for k in self.kernels[1:]:
            g = k.generator_matrix
            G = _kron(G, torch.eye(g.shape[-1], dtype=torch.float64)) + _kron(torch.eye(G.shape[-1], dtype=torch.float64), g)
        return G

    def hyperparameter_leaves(self, device="cpu"):
        return [k.hyperparameter_leaves(device) for k in self.kernels]

    def _parts(self, dt, leaves=None):
        lv = [None] * len(self.kernels) if leaves is None else leaves
        parts = [k._parts(dt, l) for k, l in zip(self.kernels, lv)]
        A, P = parts[0][0], parts[0][1]
        for a, p, _, _ in parts[1:]:
            A, P = _kron(A, a), _kron(P, p)
        inexact = [i for i, pt in enumerate(parts) if not pt[3]]
        if not inexact:
            return A, P, torch.zeros_like(A), True
        if len(inexact) == 1:
            g = inexact[0]
            Q = None
            for i, (_, p, qt, _) in enumerate(parts):
                f = qt if i == g else p
                Q = f if Q is None else _kron(Q, f)
            return A, P, Q, False
        M = None
        for a, p, _, ex in parts:
            m = p if ex else a @ p @ a.transpose(-1, -2)
            M = m if M is None else _kron(M, m)
        return A, P, P - M, False

    def _emission_row(self):
        h = self.kernels[0]._emission_row()
        for k in self.kernels[1:]:
            h = torch.kron(h, k._emission_row())
        return h

    def _terms(self):
        factors = []
        for k in self.kernels:
            t = k._terms()
            if t is None or len(t) != 1:
                return None     # a Sum child: not a product of primitive factors
            factors.extend(t[0])
        return [factors] if len(factors) <= 3 else None

    def _terms_t(self, leaves):
        factors = []
        for k, lv in zip(self.kernels, leaves):
            t = k._terms_t(lv)
            if t is None or len(t) != 1:
                return None
            factors.extend(t[0])
        return [factors] if len(factors) <= 3 else None

    def hyperparameter_values(self):
        return [k.hyperparameter_values() for k in self.kernels]

    def assign_hyperparameters(self, values):
        _assign_children(self.kernels, values)


class IndependentMultiOutput(Sum):
    """sde_kernel.py:826-880: independent processes stacked into one state, one output per child.  The prior state-space model is that of
    Sum over the same children (block-diagonal A, Q, Pinf: the packed and the wide construction are inherited); only the emission
    differs -- block-diagonal [len(kernels), state_dim] where Sum adds the children's rows up."""

    def __init__(self, kernels, jitter=0.0):
        super().__init__(kernels, jitter)
        self.output_dim = len(self.kernels)

    def _emission_matrix(self):
        """[output_dim, state_dim]: row j holds child j's emission row at child j's slice of the state."""
        H = torch.zeros((len(self.kernels), self.state_dim), dtype=torch.float64)
        o = 0
        for j, k in enumerate(self.kernels):
            H[j, o:o + k.state_dim] = k._emission_row()
            o += k.state_dim
        return H

    def generate_emission_model(self, time_points):
        return _emission_model(self._emission_matrix(), time_points)


class FactorAnalysisKernel(IndependentMultiOutput):
    """sde_kernel.py:881-941: output_dim observable processes that mix L = len(kernels) independent latent GPs linearly,
        f_p(t) = sum_l W_pl(t) g_l(t),   W(t) = A(t) B,
    with A a known, possibly time-dependent weight matrix and B [L, L] the loading matrix (identity at construction).  The state and
    the prior state-space model are those of IndependentMultiOutput over the same children (`latent_components`); only the emission
    differs: W(t) (H_1 (+) ... (+) H_L), materialised (the reference composes two emission models).

    weight_function: a callable t [..., N] -> [..., N, output_dim, L], or a tensor A [output_dim, L] for time-invariant weights (the
    emission model then carries `constant_matrix`).  `trainable` is kept for the reference's signature: B is assigned through
    assign_loading_matrix by whatever optimiser the caller runs (FactorAnalysisSparseCVI.loading_grad gives its gradient)."""

    def __init__(self, weight_function, kernels, output_dim, trainable=True, jitter=0.0):
        kernels = list(kernels)
        for k in kernels:
            if isinstance(k, PiecewiseKernel):
                raise NotImplementedError("FactorAnalysisKernel does not take PiecewiseKernel children: the stacked state is a Sum of "
                                          "stationary kernels")
            if isinstance(k, LatentExponentiallyGenerated):
                raise NotImplementedError("FactorAnalysisKernel does not take LEG children: one scalar emission row per latent")
        super().__init__(kernels, jitter)
        self.latent_components = IndependentMultiOutput(kernels, jitter)
        self.latent_dim = len(kernels)
        self.output_dim = int(output_dim)
        self.trainable = bool(trainable)
        if callable(weight_function):
            self._A, self._Afn = None, weight_function
        else:
            A = torch.as_tensor(weight_function, dtype=torch.float64)
            if tuple(A.shape) != (self.output_dim, self.latent_dim):
                raise ValueError(f"constant weights must be [output_dim, n_latents] = [{self.output_dim}, {self.latent_dim}], got "
                                 f"{tuple(A.shape)}")
            self._A, self._Afn = A, None
        self._B = torch.eye(self.latent_dim, dtype=torch.float64)
        self.loading_version = 0          # moves with every assign_loading_matrix: what caches of W are kept for

    @property
    def loading_matrix(self):
        return self._B

    def assign_loading_matrix(self, B):
        B = torch.as_tensor(B, dtype=torch.float64).detach().to("cpu")
        if tuple(B.shape) != (self.latent_dim, self.latent_dim):
            raise ValueError(f"the loading matrix is [{self.latent_dim}, {self.latent_dim}], got {tuple(B.shape)}")
        self._B = B.clone()
        self.loading_version += 1

    @property
    def constant_weights(self):
        """True when A does not depend on time."""
        return self._A is not None

    def base_weights(self, time_points):
        """A(t): [P, L] for time-invariant weights, else [..., N, P, L], on the device of time_points."""
        if self._A is not None:
            return self._A.to(time_points.device)
        A = torch.as_tensor(self._Afn(time_points), dtype=torch.float64).to(time_points.device)
        if tuple(A.shape) != tuple(time_points.shape) + (self.output_dim, self.latent_dim):
            raise ValueError(f"weight_function must return {tuple(time_points.shape) + (self.output_dim, self.latent_dim)}, got "
                             f"{tuple(A.shape)}")
        return A

    def weights(self, time_points):
        """W(t) = A(t) B: [P, L] for time-invariant weights, else [..., N, P, L]."""
        return self.base_weights(time_points) @ self._B.to(time_points.device)

    def generate_emission_model(self, time_points):
        H = self._emission_matrix().to(time_points.device)          # H_1 (+) ... (+) H_L  [L, D]
        W = self.weights(time_points)
        if self._A is not None:
            return _emission_model(W @ H, time_points)
        return EmissionModel((W @ H).contiguous())


class SparseSpatioTemporalKernel(IndependentMultiOutput):
    """spatio_temporal_variational.py:45-106: k((x, t), (x', t')) = k_s(x, x') k_t(t, t') with space marginalised to the Ms inducing
    locations Z_s -- f(Z_s, .) = chol(K_s(Z_s, Z_s)) [H_t s_1(.), ..., H_t s_Ms(.)] with s_j independent copies of the time kernel's
    state, state_dim = Ms d_t.  kernel_space: a vidp_amd.space_kernels kernel; jitter is added to K_s(Z_s, Z_s) before its
    factorisation (0, as in the reference, by default)."""

    def __init__(self, kernel_space, kernel_time, inducing_space, jitter=0.0):
        inducing_space = torch.as_tensor(inducing_space, dtype=torch.float64)
        if inducing_space.dim() != 2:
            raise NotImplementedError("one set of spatial inducing points [Ms, p]; batched inducing points are not supported")
        if getattr(kernel_time, "output_dim", 1) != 1:
            raise ValueError("the time kernel must have one output")
        self.kernel_space, self.kernel_time, self.inducing_space = kernel_space, kernel_time, inducing_space
        self.space_jitter = float(jitter)
        super().__init__([kernel_time] * int(inducing_space.shape[0]))
        self._chol = None

    def _time_emission_row(self, device):
        """H_t [d_t]; the time kernel's emission must not depend on time."""
        H = self.kernel_time.generate_emission_model(torch.zeros(1, dtype=torch.float64)).constant_matrix
        if H is None:
            raise NotImplementedError("the time kernel's emission matrix must be time-invariant")
        return H.reshape(-1).to(device, torch.float64)

    def chol_space(self, device=None):
        """chol(K_s(Z_s, Z_s) + jitter I) [Ms, Ms]."""
        if self._chol is None:
            Z = self.inducing_space
            Kzz = self.kernel_space.K(Z) + self.space_jitter * torch.eye(Z.shape[0], dtype=torch.float64, device=Z.device)
            self._chol = torch.linalg.cholesky(Kzz)
        return self._chol if device is None else self._chol.to(device)

    def generate_emission_model(self, time_points):
        """chol(K_zz) @ blockdiag(H_t) [Ms, Ms d_t], the same at every time point."""
        dev = time_points.device
        return _emission_model(self.chol_space(dev) @ self._emission_matrix().to(dev), time_points)

    def spatial_features(self, x):
        """(a [N, Ms], k_s(x, x) - |a|^2 [N]) with a = chol(K_zz)^-1 k_s(Z_s, x): the spatial half of the projection of f(x, t) onto
        the state and the spatial conditional variance."""
        L = self.chol_space(x.device)
        Kzx = self.kernel_space.K(self.inducing_space.to(x.device), x)
        a = torch.linalg.solve_triangular(L, Kzx, upper=False).transpose(-1, -2).contiguous()
        return a, self.kernel_space.K_diag(x) - (a * a).sum(-1)

    def state_to_space_conditional_projection(self, inputs):
        """E[f(x, t) | s(t)] = P s(t): P = k_s(x, Z_s) chol(K_zz)^-T blockdiag(H_t), [N, 1, state_dim]; inputs [N, p + 1], time last."""
        a, _ = self.spatial_features(inputs[..., :-1])
        Ht = self._time_emission_row(inputs.device)
        return (a[..., :, None] * Ht).reshape(tuple(a.shape[:-1]) + (1, self.state_dim))


class PiecewiseKernel:
    """kernels/piecewise_stationary.py:28-289: an SDE kernel whose dynamics are those of kernels[r] on the r-th of the K + 1 regions the
    K sorted change points c_0 <= ... <= c_{K-1} cut the time axis into, r(t) = #{c_k <= t} (a point on a change point belongs to the
    region after it).  The children are of one class and differ only in their parameter values (lengthscales / rates, variances, state
    means); they may be Sum / Product trees.

    The transition t_k -> t_k+1 of a state-space model is governed by the region of its LEFT end: A_k = A_r(t_k+1 - t_k),
    Q_k = Pinf_r - A_k Pinf_r A_k^T + jitter, b_k = (I - A_k) m_r with r = r(t_k).  As in the reference, state-space models built by
    marginalising the process to time points are only valid if no transitions cross a change point: put the change points on time
    points of the grid (two grids that cut a region differently around a change point otherwise define different priors).

    The first state has covariance Pinf_r(t_0) + jitter and mean ZERO: the reference's PiecewiseKernel inherits
    SDEKernel.initial_mean, which returns zeros whatever the children's state means are.

    state_dim <= 8 and a tree mfgm_kernel_terms expresses: state_space_model is one launch of mfgm_packed_piecewise_ssm (the kernel
    looks the regions up itself); otherwise the torch closed forms of the children, selected by region, and the wide sweeps."""

    def __init__(self, kernels, change_points, output_dim=1, jitter=0.0):
        kernels = list(kernels)
        if not kernels:
            raise ValueError("There must be at least one child kernel.")
        if not all(isinstance(k, StationaryKernel) for k in kernels):
            raise TypeError("can only combine Kernel instances")
        if not all(type(k) is type(kernels[0]) for k in kernels):
            raise TypeError("can only combine kernels from the same class")
        if output_dim != 1 or any(k.output_dim != 1 for k in kernels):
            raise ValueError("only output_dim == 1 kernels are on the hot path")
        cp = torch.as_tensor(change_points, dtype=torch.float64).detach().reshape(-1).cpu()
        if len(kernels) != cp.numel() + 1:
            raise ValueError(f"{cp.numel()} change points need {cp.numel() + 1} kernels, got {len(kernels)}")
        if cp.numel() > 1 and bool((cp[1:] < cp[:-1]).any()):
            raise ValueError("the change points must be sorted")
        if any(_tree_jitter(k) for k in kernels):
            raise ValueError("a jitter on a child of PiecewiseKernel is not supported; set it on the PiecewiseKernel")
        structs = [_structure(k) for k in kernels]
        if any(st != structs[0] for st in structs[1:]):
            raise ValueError("the children of PiecewiseKernel must have the same structure (they may differ in parameter values only)")
        self.kernels, self.change_points = kernels, cp
        self.num_change_points = int(cp.numel())
        self.output_dim, self.jitter = 1, float(jitter)
        self._state_dim = kernels[0].state_dim

    @property
    def state_dim(self):
        return self._state_dim

    # -- regions ------------------------------------------------------------------------------------------------------------------------
    def split_time_indices(self, time_points):
        """Index 0 .. K of the region every time point lies in (any shape): #{c_k <= t}, i.e. searchsorted(..., "right") - 1 on the
        change points augmented with -inf and +inf (piecewise_stationary.py:126-143)."""
        t = torch.as_tensor(time_points, dtype=torch.float64)
        return torch.searchsorted(self.change_points.to(t.device), t.contiguous(), right=True)

    def _by_region(self, per_child, time_points):
        table = torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in per_child])
        r = self.split_time_indices(time_points)
        return table.to(r.device)[r]

    def steady_state_covariances(self, time_points):
        """Pinf of the kernel active at each time point, [..., d, d]."""
        return self._by_region([k.steady_state_covariance for k in self.kernels], time_points)

    def feedback_matrices(self, time_points):
        """F of the kernel active at each time point, [..., d, d]."""
        return self._by_region([k.feedback_matrix for k in self.kernels], time_points)

    def state_means(self, time_points):
        """State mean of the kernel active at each time point, [..., d]."""
        return self._by_region([k.state_mean for k in self.kernels], time_points)

    # -- transitions: torch closed forms of the children, selected by the region of the transition's left end ---------------------------
    def transition_statistics_at(self, transition_times, time_deltas):
        """(A, Q) of the transitions that start at transition_times and last time_deltas (any shape, unordered): every child's closed
        forms on all gaps, then a selection by region (no host synchronisation, K + 1 times the arithmetic)."""
        r = self.split_time_indices(transition_times)[..., None, None]
        A = Q = None
        for i, k in enumerate(self.kernels):
            Ai, Qi = k.transition_statistics_local(time_deltas)
            A, Q = (Ai, Qi) if A is None else (torch.where(r == i, Ai, A), torch.where(r == i, Qi, Q))
        return A, Q + self.jitter * torch.eye(self.state_dim, dtype=Q.dtype, device=Q.device)

    def transition_statistics(self, transition_times, time_deltas):
        """piecewise_stationary.py:206-228.  Only valid if no transition crosses a change point."""
        return self.transition_statistics_at(transition_times, time_deltas)

    def state_transitions(self, transition_times, time_deltas):
        """piecewise_stationary.py:180-204.  Only valid if no transition crosses a change point."""
        return self.transition_statistics_at(transition_times, time_deltas)[0]

    def state_offsets(self, transition_times, time_deltas):
        """b = (I - A) m of the region of the transition's left end (piecewise_stationary.py:248-271)."""
        A = self.state_transitions(transition_times, time_deltas)
        m = self.state_means(transition_times).to(A.device)
        return m - (A @ m[..., None])[..., 0]

    def initial_covariance(self, initial_time_point):
        """Pinf + jitter of the kernel active at the time of the first state: [d, d] for one time ([1] or a scalar), batch_shape + [d, d]
        for batch_shape + [1] (piecewise_stationary.py:111-124)."""
        t = torch.as_tensor(initial_time_point, dtype=torch.float64)
        P = self.steady_state_covariances(t) + self.jitter * torch.eye(self.state_dim, dtype=torch.float64, device=t.device)
        return P[..., 0, :, :] if t.dim() >= 1 else P

    def initial_mean(self, batch_shape=()):
        """Zeros, as in the reference (SDEKernel.initial_mean; the children's state means enter the offsets only)."""
        return torch.zeros(tuple(batch_shape) + (self.state_dim,), dtype=torch.float64)

    def _emission_row(self):
        return self.kernels[0]._emission_row()

    def generate_emission_model(self, time_points):
        """The children's common H, the same at every time point."""
        return _emission_model(self._emission_row()[None], time_points)

    # -- the prior state-space model ----------------------------------------------------------------------------------------------------
    def _terms(self):
        terms = [k._terms() for k in self.kernels] if self.state_dim <= 8 else None
        return None if terms is None or terms[0] is None or len(terms[0]) > 8 else terms

    def _terms_struct(self, device):
        """(mfgm_piecewise_terms, the device tensor that holds its tables): one host-to-device copy."""
        terms = self._terms()
        if terms is None:
            raise ValueError("the piecewise kernel takes up to 8 terms of up to 3 primitive factors and state_dim <= 8")
        K1, d = len(self.kernels), self.state_dim
        pw = _lib.PiecewiseTerms()
        base = self.kernels[0]._terms_struct(terms[0])
        base.jitter = self.jitter
        pw.base, pw.nregion = base, K1
        rate, var = torch.zeros((K1, 8, 3), dtype=torch.float64), torch.zeros((K1, 8, 3), dtype=torch.float64)
        mean = torch.zeros((K1, 8), dtype=torch.float64)
        for r, (k, tr) in enumerate(zip(self.kernels, terms)):
            for c, factors in enumerate(tr):
                for f, (_, ra, va) in enumerate(factors):
                    rate[r, c, f], var[r, c, f] = ra, va
            mean[r, :d] = k.state_mean
        host = torch.cat([rate.reshape(-1), var.reshape(-1), mean.reshape(-1), self.change_points])
        tab = host.to(device)
        n = K1 * 24
        pw.rate, pw.var, pw.mean = tab.data_ptr(), tab[n:].data_ptr(), tab[2 * n:].data_ptr()
        pw.change_points = tab[2 * n + K1 * 8:].data_ptr() if K1 > 1 else None
        return pw, tab

    # VIDP_PIECEWISE_TORCH=1: the region-selected torch closed forms also where the HIP kernel applies (the tests compare the two routes)
    def state_space_model(self, time_points, plan=None):
        """Prior SSM at the sorted time points [..., T], each chain with its own grid.  Only valid if no transition crosses a change
        point (a crossing transition is governed by its left end)."""
        t, bs = _flat(time_points, 1)
        B, T = t.shape
        if plan is None:
            plan = Plan(B, T, self.state_dim, device=t.device)
        if self._terms() is None or os.environ.get("VIDP_PIECEWISE_TORCH", "0") == "1":
            return self._state_space_model_torch(t, bs, plan)
        pw, tab = self._terms_struct(t.device)
        ssm = _model_from_packed(plan, plan.piecewise_ssm(pw, t), bs)
        ssm._piecewise_tables = tab      # the launch reads them: kept with the model
        return ssm

    def _state_space_model_torch(self, t, bs, plan):
        """StationaryKernel._state_space_model_wide on the region-selected closed forms."""
        A, Q = self.transition_statistics_at(t[:, :-1], t[:, 1:] - t[:, :-1])
        try:
            return _model_from_torch(A, Q, self.state_means(t[:, :-1]), self.initial_mean().to(t.device),
                                     self.initial_covariance(t[:, :1]), plan, bs)
        except ArithmeticError as e:
            raise ArithmeticError(_NOT_PD) from e

    # -- hyper-parameters as leaves of a torch graph ------------------------------------------------------------------------------------
    def hyperparameter_leaves(self, device="cpu"):
        """One entry per region: the children's hyperparameter_leaves."""
        return [k.hyperparameter_leaves(device) for k in self.kernels]

    def differentiable_ssm(self, time_points, leaves=None, plan=None):
        """(tape.TapeSSM, leaves): the prior SSM at the sorted time points [T] (one chain, d <= 8) as a differentiable function of the
        per-region hyper-parameter leaves -- the children's differentiable _parts on all gaps, selected by the region of each
        transition's left end; a region that holds no left end and not the first point gets a gradient of exactly zero."""
        t = time_points.reshape(-1)
        dev, d = t.device, self.state_dim
        if leaves is None:
            leaves = self.hyperparameter_leaves(dev)
        r = self.split_time_indices(t)
        rl, dt = r[:-1, None, None], t[1:] - t[:-1]
        A = Qt = Pinf0 = None
        exact = True
        for i, (k, lv) in enumerate(zip(self.kernels, leaves)):
            Ai, Pi, Qi, ex = k._parts(dt, lv)
            exact = exact and ex
            Pi = Pi.expand(d, d)
            A, Qt = (Ai, Qi) if A is None else (torch.where(rl == i, Ai, A), torch.where(rl == i, Qi, Qt))
            Pinf0 = Pi if Pinf0 is None else torch.where(r[0] == i, Pi, Pinf0)
        return _tape_model(A, Qt, exact, Pinf0, self.state_means(t[:-1]), self.initial_mean().to(dev), self.jitter, plan), leaves


def _tree_jitter(kernel):
    """Whether the kernel or any kernel below it carries a jitter."""
    return kernel.jitter != 0.0 or any(_tree_jitter(k) for k in getattr(kernel, "kernels", []))


def _structure(kernel):
    """What the children of a PiecewiseKernel must share: the class tree, the state dimension, the emission row and, where the tree
    has them, the kinds of the terms' factors -- everything of _terms() but the rates and variances."""
    terms = kernel._terms() if kernel.state_dim <= 8 else None
    kinds = None if terms is None else [[kind for kind, _, _ in factors] for factors in terms]
    tree = lambda k: (type(k).__name__, [tree(c) for c in getattr(k, "kernels", [])])
    return tree(kernel), kernel.state_dim, kernel._emission_row().tolist(), kinds
