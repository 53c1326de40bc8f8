"""
Gradients of the log marginal likelihood with respect to the kernel's hyper-parameters, by Fisher's identity:

    d/dh log Z(h) = E_post[d/dh log p_h(x)],

and the prior log density of a Gauss-Markov chain is a sum over the transitions of terms quadratic in (x_k, x_k+1), so the expectation
needs the posterior pairwise moments (mu, Sigma_tt, Sigma_{t+1,t}) only -- what one selected inverse on the factorisation that
log_likelihood() makes anyway returns.  With moments centred on the prior state mean,

    S = Sigma_k + mu_k mu_k^T,  S' = Sigma_k+1 + mu_k+1 mu_k+1^T,  C = Sigma_{k+1,k} + mu_k+1 mu_k^T,
    M = S' - A C^T - C A^T + A S A^T,
    G_Q = 1/2 (Q^-1 M Q^-1 - Q^-1),   G_A = Q^-1 (C - A S),   G_P0 = 1/2 (P0^-1 S_0 P0^-1 - P0^-1),
    d log Z = <G_P0, dP0> + sum_k <G_Q,k, dQ_k> + <G_A,k, dA_k>.

A transition whose Q is exactly zero (zero gap, Constant) carries no score; it has none when dA != 0 there (a noise-free
HarmonicOscillator term without jitter), which is rejected before anything is launched.

Two routes:
  native    kernels with `_terms()` and state_dim <= 8: one launch of mfgm_packed_kernel_score (csrc/mfgm_score.h) gives the score
            with respect to every factor's (rate, var); the chain rule to the leaves is one scalar autograd call on the host.
  fallback  any other kernel with `_parts(dt, leaves)` (state_dim > 8, LatentExponentiallyGenerated): the cotangents as batched torch
            expressions on the unpacked moments (vidp_amd.linalg for the d x d solves), then one backward pass through `_parts`.
VIDP_NATIVE_SCORE=0 forces the fallback.
"""
import math
import os

import torch

from . import _lib, linalg
from ._lib import FULL, SYM, VEC

_NO_SCORE = ("a HarmonicOscillator term without process noise has a transition that depends on its period but an exactly-zero Q: "
             "its likelihood has no score with respect to the period; set a jitter on the kernel")


def flatten(leaves):
    """The tensors (or floats) of a hyperparameter_leaves() / hyperparameter_values() structure, depth first, dict entries in order."""
    if isinstance(leaves, dict):
        return list(leaves.values())
    out = []
    for l in leaves:
        out.extend(flatten(l))
    return out


def unflatten(like, flat):
    """The structure of `like` filled from the list `flat` (consumed from the front)."""
    if isinstance(like, dict):
        return {k: flat.pop(0) for k in like}
    return [unflatten(l, flat) for l in like]


def check_supported(kernel):
    """The kernels the hyper-parameter score covers: trees of the stationary kernels with a single output."""
    from .kernels import IndependentMultiOutput, PiecewiseKernel, StationaryKernel
    if isinstance(kernel, (PiecewiseKernel, IndependentMultiOutput)) or not isinstance(kernel, StationaryKernel):
        raise NotImplementedError(f"hyper-parameter gradients are not implemented for {type(kernel).__name__}")


def _grads_of(leaves, objective):
    """Leaf gradients of the scalar `objective` in the structure of `leaves`, as 0-dim (or matrix) CPU fp64 tensors."""
    flat = flatten(leaves)
    grads = torch.autograd.grad(objective, flat, allow_unused=True)
    out = [torch.zeros_like(l) if g is None else g for l, g in zip(flat, grads)]
    return unflatten(leaves, [g.detach().to("cpu", torch.float64) for g in out])


def native_route(kernel, plan):
    """Whether the score of this kernel on this plan is one launch of mfgm_packed_kernel_score."""
    if os.environ.get("VIDP_NATIVE_SCORE", "1") == "0" or kernel.state_dim > 8 or plan.d != kernel.state_dim or plan.wide:
        return False
    terms = kernel._terms()
    return terms is not None and len(terms) <= 8 and plan.device.type == "cuda"


def _check_terms(kernel, terms):
    exact = (_lib.FACTOR_CONSTANT, _lib.FACTOR_HARMONIC)
    if kernel.jitter != 0.0:
        return
    for factors in terms:
        kinds = [k for k, _, _ in factors]
        if all(k in exact for k in kinds) and _lib.FACTOR_HARMONIC in kinds:
            raise ValueError(_NO_SCORE)


def score_native(kernel, plan, time_deltas, moments):
    """Kernel gradients (structure of hyperparameter_leaves(), CPU) from the packed centred moments, summed over the chains."""
    from .kernels import _NOT_PD
    terms = kernel._terms()
    _check_terms(kernel, terms)
    g = plan.kernel_score(kernel._terms_struct(terms), time_deltas, moments["x"], moments["Sig"], moments["Sub"])
    try:
        plan.check_info()
    except ArithmeticError as e:
        raise ArithmeticError(_NOT_PD) from e
    g = g.sum(0).cpu()
    leaves = kernel.hyperparameter_leaves("cpu")
    objective = torch.zeros((), dtype=torch.float64)
    for c, factors in enumerate(kernel._terms_t(leaves)):
        for f, (_, rate, var) in enumerate(factors):
            objective = objective + rate * g[c, f, 0] + var * g[c, f, 1]
    return _grads_of(leaves, objective)


def _sym_solve(chol, M):
    """K^-1 M K^-1 for K = chol chol^T and symmetric M."""
    X = linalg.cholesky_solve(M, chol)
    return linalg.cholesky_solve(X.transpose(-1, -2).contiguous(), chol)


def cotangents(A, P, Qterm, jitter, mu, Sig, Sub):
    """(G_A [B, T-1, d, d], G_Q [B, T-1, d, d], G_P0 [B, d, d]) from natural centred moments mu [B, T, d], Sig [B, T, d, d] and
    Sub [B, T-1, d, d] = Sigma_{t+1,t}; transitions whose Q = Qterm + jitter I is exactly zero get zero cotangents."""
    d = mu.shape[-1]
    eye = torch.eye(d, dtype=torch.float64, device=mu.device)
    S = Sig + mu[..., :, None] * mu[..., None, :]
    P0 = (P + jitter * eye).expand(mu.shape[0], d, d).contiguous()
    c0 = linalg.cholesky(P0)
    G_P0 = 0.5 * (_sym_solve(c0, S[:, 0].contiguous()) - linalg.spd_inverse(chol=c0))
    if mu.shape[1] == 1:
        return None, None, G_P0
    Q = Qterm + jitter * eye
    zero = (Q == 0).all(dim=-1).all(dim=-1)[..., None, None]
    chol = linalg.cholesky(torch.where(zero, eye, Q).contiguous())
    C = Sub + mu[:, 1:, :, None] * mu[:, :-1, None, :]
    Sk, Sn = S[:, :-1], S[:, 1:]
    W = C - A @ Sk
    M = Sn - A @ C.transpose(-1, -2) - W @ A.transpose(-1, -2)
    M = 0.5 * (M + M.transpose(-1, -2))
    G_Q = 0.5 * (_sym_solve(chol, M.contiguous()) - linalg.spd_inverse(chol=chol))
    G_A = linalg.cholesky_solve(W.contiguous(), chol)
    keep = (~zero).to(torch.float64)
    return G_A * keep, G_Q * keep, G_P0


def score_fallback(kernel, plan, time_deltas, moments):
    """The same gradients through torch: cotangents from the unpacked moments, one backward pass through kernel._parts."""
    B, T, d = plan.B, plan.T, plan.d
    mu = plan.unpack(VEC, moments["x"])
    Sig = plan.unpack(SYM, moments["Sig"])
    Sub = plan.unpack(FULL, moments["Sub"], T - 1) if T > 1 else None
    dev = mu.device
    dts = time_deltas if T > 1 else torch.zeros((B, 0), dtype=torch.float64, device=dev)
    with torch.no_grad():
        A, P, Qterm, exact = kernel._parts(dts)
        if exact and kernel.jitter == 0.0 and T > 1 and bool((dts != 0).any()) and bool(((A - torch.eye(d, dtype=A.dtype, device=dev)) != 0).any()):
            raise ValueError(_NO_SCORE)
        G_A, G_Q, G_P0 = cotangents(A, P, Qterm, kernel.jitter, mu, Sig, Sub)
    leaves = kernel.hyperparameter_leaves(dev)
    Ah, Ph, Qh, _ = kernel._parts(dts, leaves)
    objective = (G_P0.sum(0) * Ph).sum()
    if T > 1:
        objective = objective + (G_A * Ah).sum() + (G_Q * Qh).sum()
    return _grads_of(leaves, objective)


def precheck(kernel):
    """The checks that need the kernel alone (supported class, no noise-free HarmonicOscillator term without jitter): the models run
    them before they build the prior, so that a refused kernel launches nothing."""
    check_supported(kernel)
    terms = kernel._terms() if kernel.state_dim <= 8 else None
    if terms is not None:
        _check_terms(kernel, terms)


def kernel_score(kernel, kalman, time_points):
    """(log likelihood, kernel gradients, moments, displacement) of a BaseKalmanFilter whose prior is `kernel` at `time_points`: one
    factorisation, one selected inverse and one score pass.  The caller has run precheck(kernel) before it built the prior."""
    plan = kalman.prior_ssm.plan
    native = native_route(kernel, plan)
    ll, moments, disp = kalman.log_likelihood_and_moments()
    t = time_points.reshape(plan.B, plan.T)
    dts = (t[:, 1:] - t[:, :-1]).contiguous() if plan.T > 1 else None
    grads = (score_native if native else score_fallback)(kernel, plan, dts, moments)
    return ll, grads, moments, disp


# -- unconstrained parametrisations of the positive scalars (KernelHyperTrainer) ---------------------------------------------------------
def softplus(u):
    """log(1 + e^u), the forward map of gpflow's default `positive()` bijector."""
    return max(u, 0.0) + math.log1p(math.exp(-abs(u)))


def softplus_inverse(x):
    """u with softplus(u) = x, x > 0."""
    return x + math.log(-math.expm1(-x))


def softplus_jacobian(u):
    """d softplus / du = sigmoid(u)."""
    return 1.0 / (1.0 + math.exp(-u)) if u >= 0 else math.exp(u) / (1.0 + math.exp(u))


TRANSFORMS = {
    # name: (forward, inverse, d forward / d u)
    "softplus": (softplus, softplus_inverse, softplus_jacobian),
    "log": (math.exp, math.log, math.exp),
}
