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

The sparse CVI model (SparseCVIGaussianProcess.elbo_and_grad) differentiates its ELBO at fixed sites with the
same two routes for the chain part, fed with the moments displaced by a Fisher-vector product, plus a part through the conditionals
of the data points: one launch of mfgm_sparse_cond_score (csrc/mfgm_sparse_score.h) natively, autograd through `_parts` otherwise
(`sparse_elbo_grad`; VIDP_NATIVE_SPARSE_SCORE=0 forces the torch route).  PanelSparseCVI.elbo_and_grad is the
same decomposition with a leading series axis, summed over the series: one batched Fisher-vector product, one batched chain score and
one launch of mfgm_panel_cond_score (csrc/mfgm_panel_score.h) on the packed marginals of the B-chain plan (`panel_elbo_grad`).
"""
import math
import os

import torch

from . import _lib, linalg
from ._lib import FULL, SYM, VEC
from .conditionals import interval_gaps

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


def _leaves_from_score(kernel, g):
    """The chain rule from a score g [8, 3, 2] (CPU) with respect to every factor's (rate, var) to the kernel's leaves: one scalar
    autograd call on the host."""
    leaves = kernel.hyperparameter_leaves("cpu")
    objective = torch.zeros((), dtype=torch.float64)
    for c, factors in enumerate(kernel._terms_t(leaves)):
        for f, (_, rate, var) in enumerate(factors):
            objective = objective + rate * g[c, f, 0] + var * g[c, f, 1]
    return _grads_of(leaves, objective)


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
    return _leaves_from_score(kernel, g.sum(0).cpu())


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


# -- the sparse CVI bound at fixed sites ----------------------------------------------------------------------------
def _add_grads(like, *parts):
    """Sum of gradient structures of the shape of `like`."""
    flats = [flatten(p) for p in parts]
    return unflatten(like, [sum(g[1:], g[0]) for g in zip(*flats)])


def overlap_add(n1, n2):
    """Pair sites (n1 [..., M + 1, 2d], n2 [..., M + 1, 2d, 2d]) -> the chain's (lin [..., M, d], diag [..., M, d, d],
    sub [..., M - 1, d, d]) in mfgm_sparse_theta's convention: site t + 1 starts at inducing state t, site t ends there; sub takes
    twice the lower-left block.  Leading axes (the panel's series) pass through."""
    d = n1.shape[-1] // 2
    lin = n1[..., 1:, :d] + n1[..., :-1, d:]
    diag = n2[..., 1:, :d, :d] + n2[..., :-1, d:, d:]
    sub = 2.0 * n2[..., 1:-1, d:, :d]
    return lin, diag, sub


def conditional_part_torch(kernel, gap_lo, gap_hi, a, b, mu_pair, Sig_pair, idx, M):
    """Gradients of  sum_i a_i fmu_i + b_i fvar_i  at fixed pair moments through the conditionals, by autograd through kernel._parts:
    Q_mp = Q2 + A2 Q1 A2^T, x = Q_mp^-1 A2 Q1 h, y = h - A2^T x, w = (A1^T y, x), c = h^T Q1 y.  mu_pair [N, 2d], Sig_pair [N, 2d, 2d]:
    the pair marginals of the points' intervals, whose prior padding at the two ends is replaced by Pinf(leaves) + jitter I here."""
    from . import tape
    dev = gap_lo.device
    d = kernel.state_dim
    leaves = kernel.hyperparameter_leaves(dev)
    eye = torch.eye(d, dtype=torch.float64, device=dev)
    A1, P, Q1, _ = kernel._parts(gap_lo, leaves)
    A2, _, Q2, _ = kernel._parts(gap_hi, leaves)
    Q1, Q2 = Q1 + kernel.jitter * eye, Q2 + kernel.jitter * eye
    h = kernel._emission_row().to(dev)[:, None]
    u = Q1 @ h
    Qmp = Q2 + A2 @ Q1 @ A2.transpose(-1, -2)
    x = tape.cholesky_solve(tape.cholesky(0.5 * (Qmp + Qmp.transpose(-1, -2))), A2 @ u)
    y = h - A2.transpose(-1, -2) @ x
    w = torch.cat([A1.transpose(-1, -2) @ y, x], dim=-2)[..., 0]
    c = (u * y).sum(dim=(-1, -2))
    P0 = P + kernel.jitter * eye
    lo, hi = (idx == 0)[:, None, None], (idx == M)[:, None, None]
    S = Sig_pair.clone()
    S[:, :d, :d] = torch.where(lo, P0, S[:, :d, :d])
    S[:, d:, d:] = torch.where(hi, P0, S[:, d:, d:])
    fmu = (w * mu_pair).sum(-1)
    fvar = c + (w[:, None, :] @ S @ w[:, :, None])[:, 0, 0]
    return _grads_of(leaves, (a * fmu).sum() + (b * fvar).sum())


def conditional_part_native(kernel, plan, data, gap_lo, gap_hi, a, b, marg):
    """The same gradients from one launch of mfgm_sparse_cond_score on the fused route's data (csrc/mfgm_sparse_score.h)."""
    import ctypes
    from .kernels import _NOT_PD
    from .packed import _ptr, _stream
    lib = plan.lib
    ws = data.get("score_ws")
    if ws is None:
        ws = data["score_ws"] = torch.empty(int(lib.mfgm_sparse_cond_score_workspace_doubles(data["N"])), dtype=torch.float64, device=a.device)
    terms = kernel._terms()
    score = torch.empty((8, 3, 2), dtype=torch.float64, device=a.device)
    # the entry point takes whole chains only and says so by m_hi <= 0; the model's struct names its range (0, M + 1) explicitly
    sd, src = _lib.SparseData(), data["struct"]
    for name, _ in _lib.SparseData._fields_:
        setattr(sd, name, getattr(src, name))
    sd.m_lo, sd.m_hi = 0, 0
    _lib.check(lib.mfgm_sparse_cond_score(ctypes.byref(sd), ctypes.byref(kernel._terms_struct(terms)), _ptr(gap_lo), _ptr(gap_hi),
                                          _ptr(a), _ptr(b), _ptr(marg["mu"]), _ptr(marg["Sig"]), _ptr(marg["Sub"]), _ptr(score), _ptr(ws),
                                          _ptr(plan.info), _stream()), "mfgm_sparse_cond_score")
    try:
        plan.check_info()
    except ArithmeticError as e:
        raise ArithmeticError(_NOT_PD) from e
    return _leaves_from_score(kernel, score.cpu())


def sparse_native_route(model, data):
    """Whether elbo_and_grad takes the HIP route: the fused data route applies and the chain part's score is native."""
    return (data is not None and os.environ.get("VIDP_NATIVE_SPARSE_SCORE", "1") != "0"
            and native_route(model._kernel, model.dist_p.plan))


def sparse_elbo_grad(model, input_data, parts=None):
    """Exact gradient of SparseCVIGaussianProcess.classic_elbo with respect to the kernel's hyper-parameters at fixed sites (structure of
    hyperparameter_leaves(), CPU fp64).  With theta_p the prior's naturals on the inducing chain, theta_s the overlap-added sites, F the
    Fisher matrix of q and g^ the overlap-added CVI target sum_i (g1_i w_i, g2_i w_i w_i^T),
        dL = < eta_q - eta_p + F (g^ - theta_s), d theta_p >  +  sum_i a_i d fmu_i + b_i d fvar_i  (q fixed),
    a = g1 + 2 g2 fmu, b = g2.  The first bracket is the log-likelihood score on moments displaced by the Fisher-vector product (its
    linear component meets d theta_p's, which is zero for a zero-mean prior); the second goes through the conditionals.
    parts (a dict): receives the two chain contributions and the conditional one separately."""
    from . import tape
    kernel, lik = model._kernel, model._likelihood
    time_points, observations = input_data
    z = model.inducing_inputs
    data = model._data(input_data)
    native = sparse_native_route(model, data)
    p = model.dist_p
    pl, T, d = p.plan, p.T, p.d
    m = model._marginals()
    if data is not None:
        fmu, fvar = model._predict_f_data(data)
        y = model._own_observations(data, observations)
    else:
        fmu, fvar = model.posterior.predict_f(time_points)
        y = observations
    g1, g2 = lik.ve_gradients_expectation(fmu, fvar, y)
    g1, g2, fm = g1.reshape(-1).detach(), g2.reshape(-1).detach(), fmu.reshape(-1).detach()
    a, b = (g1 + 2.0 * g2 * fm).contiguous(), g2.contiguous()
    c = data.get("gaps") if data is not None else None
    if c is None:
        c = interval_gaps(time_points.reshape(-1), z)
        if data is not None:
            data["gaps"] = c
    idx, gap_lo, gap_hi = c
    # ---- the CVI target g^ (what update_sites accumulates at lr = 1 into zero sites) minus the sites, on the chain
    if native:
        import ctypes
        from .packed import _ptr, _stream
        t1, t2 = torch.zeros_like(model.nat1), torch.zeros_like(model.nat2)
        _lib.check(pl.lib.mfgm_sparse_site_update(ctypes.byref(data["struct"]), _ptr(g1.contiguous()), _ptr(g2.contiguous()), 1.0, _ptr(t1),
                                                  _ptr(t2), _stream()), "mfgm_sparse_site_update")
    else:
        wfull = data["keep"][1][:data["N"]] if data is not None else None
        if wfull is None:
            from .conditionals import conditional_statistics
            H = kernel.generate_emission_model(time_points).emission_matrix
            Pc, _ = conditional_statistics(time_points, z, kernel)
            wfull = (H @ Pc)[:, 0, :]
        t1 = torch.zeros_like(model.nat1).index_add_(0, idx, g1[:, None] * wfull)
        t2 = torch.zeros_like(model.nat2).index_add_(0, idx, g2[:, None, None] * wfull[:, :, None] * wfull[:, None, :])
    v_lin, v_diag, v_sub = overlap_add(t1 - model.nat1, t2 - model.nat2)
    # ---- chain part: the score on (mu, Sig + delta_diag, Sub + delta_sub), delta = F (g^ - theta_s)
    model._theta()
    tb = model._theta_bufs
    mu, cov, csub = m["mu"][None], m["Sig"][None], m["Sub"][None, :T - 1]
    _, dd, ds = tape.fisher_vector_product(pl, tb["diag"][None], tb["sub"][None, :T - 1], mu, cov, csub, v_lin[None], v_diag[None], v_sub[None])
    s = m["packed"]
    dts = (z[1:] - z[:-1]).reshape(1, -1).contiguous() if T > 1 else None
    score = score_native if native else score_fallback

    def packed_band(diag, sub):
        return pl.pack(SYM, diag.contiguous()), (pl.pack(FULL, sub.contiguous()) if T > 1 else pl.zeros(FULL))

    if parts is None:
        pd, ps = packed_band(cov + dd, csub + ds)
        chain = score(kernel, pl, dts, dict(x=s["x"], Sig=pd, Sub=ps))
    else:
        # the two brackets apart: the score is affine in the second moments, so F's share is a difference of two scores
        parts["chain_kl"] = score(kernel, pl, dts, dict(x=s["x"], Sig=s["Sig"], Sub=s["Sub"]))
        pd, ps = packed_band(cov + dd, csub + ds)
        both = score(kernel, pl, dts, dict(x=s["x"], Sig=pd, Sub=ps))
        parts["chain_fisher"] = _add_grads(both, both, unflatten(both, [-g for g in flatten(parts["chain_kl"])]))
        chain = both
    # ---- conditional part
    if native:
        cond = conditional_part_native(kernel, pl, data, gap_lo, gap_hi, a, b, m)
    else:
        mean = kernel.initial_mean(()).to(z.device, torch.float64)
        cov0 = kernel.initial_covariance(z[:1]).to(z.device, torch.float64)
        ext_m = torch.cat([mean[None], m["mu"], mean[None]])
        ext_c = torch.cat([cov0[None], m["Sig"], cov0[None]])
        zero = torch.zeros_like(cov0)[None]
        ext_s = torch.cat([zero, m["Sub"][:T - 1], zero])                   # Cov(x_hi, x_lo) of interval k
        mu_pair = torch.cat([ext_m[:-1], ext_m[1:]], dim=-1)[idx]
        top = torch.cat([ext_c[:-1], ext_s.transpose(-1, -2)], dim=-1)
        bot = torch.cat([ext_s, ext_c[1:]], dim=-1)
        Sig_pair = torch.cat([top, bot], dim=-2)[idx]
        cond = conditional_part_torch(kernel, gap_lo, gap_hi, a, b, mu_pair, Sig_pair, idx, T)
    if parts is not None:
        parts["conditional"] = cond
    return _add_grads(chain, chain, cond)


# -- the panel's bound at fixed sites ---------------------------------------------------------------------------------
def panel_native_route(model):
    """Whether PanelSparseCVI.elbo_and_grad takes the HIP route: the model's fused passes apply and the chain part's score is native."""
    return (model._native() and os.environ.get("VIDP_NATIVE_SPARSE_SCORE", "1") != "0"
            and native_route(model._kernel, model.dist_p.plan))


def conditional_part_panel_native(kernel, plan, data, gap_lo, gap_hi, a, b, packed):
    """The conditional part of every series, summed, from one launch of mfgm_panel_cond_score on the packed marginals of the B-chain
    plan (csrc/mfgm_panel_score.h)."""
    import ctypes
    from .kernels import _NOT_PD
    from .packed import _ptr, _stream
    lib = plan.lib
    ws = data.get("score_ws")
    if ws is None:
        ws = data["score_ws"] = torch.empty(int(lib.mfgm_panel_cond_score_workspace_doubles(plan.B, data["n"])), dtype=torch.float64,
                                            device=a.device)
    score = torch.empty((8, 3, 2), dtype=torch.float64, device=a.device)
    _lib.check(lib.mfgm_panel_cond_score(plan.h, ctypes.byref(data["struct"]), ctypes.byref(kernel._terms_struct(kernel._terms())),
                                         _ptr(gap_lo), _ptr(gap_hi), _ptr(a), _ptr(b), _ptr(packed["x"]), _ptr(packed["Sig"]),
                                         _ptr(packed["Sub"]), _ptr(score), _ptr(ws), _ptr(plan.info), _stream()), "mfgm_panel_cond_score")
    try:
        plan.check_info()
    except ArithmeticError as e:
        raise ArithmeticError(_NOT_PD) from e
    return _leaves_from_score(kernel, score.cpu())


def panel_elbo_grad(model, input_data, parts=None):
    """Exact gradient of PanelSparseCVI.classic_elbo with respect to the shared kernel's hyper-parameters at fixed sites, summed over
    the series (structure of hyperparameter_leaves(), CPU fp64): the decomposition of sparse_elbo_grad with a leading series axis,
        dL = sum_b < eta_q - eta_p + F_b (g^_b - theta_s,b), d theta_p >  +  sum_{b,i} a_bi d fmu_bi + b_bi d fvar_bi  (q fixed).
    The chain part is one batched score over the B chains on moments displaced by one batched Fisher-vector product; the conditional
    part one launch of mfgm_panel_cond_score natively, autograd through `_parts` on at most model.CHUNK points at a time otherwise.
    parts (a dict): receives chain_kl, chain_fisher and conditional separately."""
    from . import tape
    from .pair_sites import pair_marginals
    kernel = model._kernel
    z = model.inducing_inputs
    data = model._data(input_data)
    native = panel_native_route(model)
    pl = model.dist_p.plan
    B, T, d, n = pl.B, pl.T, pl.d, data["n"]
    r = model._predict_lik(input_data)
    g1, g2 = r["g1"].contiguous(), r["g2"].contiguous()             # exact zeros at the absent points
    a, b = (g1 + 2.0 * g2 * r["fmu"]).contiguous(), g2
    c = data.get("gaps")
    if c is None:
        _, lo, hi = interval_gaps(input_data[0].reshape(-1), z)
        c = data["gaps"] = (lo.reshape(B, n).contiguous(), hi.reshape(B, n).contiguous())
    gap_lo, gap_hi = c
    w, idx = data["w"], data["idx"]
    # ---- the CVI target g^ of every series (what update_sites accumulates at lr = 1 into zero sites) minus the sites, on the chains
    if native:
        import ctypes
        from .packed import _ptr, _stream
        t1, t2 = torch.zeros_like(model.nat1), torch.zeros_like(model.nat2)
        _lib.check(pl.lib.mfgm_panel_site_update(ctypes.byref(data["struct"]), _ptr(g1), _ptr(g2), 1.0, _ptr(t1), _ptr(t2), _stream()),
                   "mfgm_panel_site_update")
    else:
        t1, t2 = model._site_sums(data, g1, g2)
    v_lin, v_diag, v_sub = overlap_add(t1 - model.nat1, t2 - model.nat2)
    # ---- chain part: the score on (mu, Sig + delta_diag, Sub + delta_sub), delta = F (g^ - theta_s), every series at once
    s = model._marginals()["packed"]
    mu, cov, csub = pl.unpack(VEC, s["x"]), pl.unpack(SYM, s["Sig"]), pl.unpack(FULL, s["Sub"], T - 1)
    _, th_diag, th_sub = model._theta()
    _, dd, ds = tape.fisher_vector_product(pl, pl.unpack(SYM, th_diag), pl.unpack(FULL, th_sub, T - 1), mu, cov, csub, v_lin, v_diag, v_sub)
    dts = (z[1:] - z[:-1])[None].expand(B, -1).contiguous()
    score = score_native if native else score_fallback
    displaced = dict(x=s["x"], Sig=pl.pack(SYM, cov + dd), Sub=pl.pack(FULL, csub + ds))
    if parts is None:
        chain = score(kernel, pl, dts, displaced)
    else:
        # the two brackets apart: the score is affine in the second moments, so F's share is a difference of two scores
        parts["chain_kl"] = score(kernel, pl, dts, dict(x=s["x"], Sig=s["Sig"], Sub=s["Sub"]))
        chain = score(kernel, pl, dts, displaced)
        parts["chain_fisher"] = _add_grads(chain, chain, unflatten(chain, [-g for g in flatten(parts["chain_kl"])]))
    # ---- conditional part
    if native:
        cond = conditional_part_panel_native(kernel, pl, data, gap_lo, gap_hi, a, b, s)
    else:
        pm, pc = pair_marginals(model, (mu, cov, csub))
        cond = None
        for lo in range(0, B, model._rows(n)):          # the pair covariances are gathered a block of series at a time
            sl = slice(lo, lo + model._rows(n))
            rows = torch.arange(pm[sl].shape[0], device=w.device)[:, None]
            flat = lambda x: x[sl].reshape(-1)
            part = conditional_part_torch(kernel, flat(gap_lo), flat(gap_hi), flat(a), flat(b), pm[sl][rows, idx[sl]].reshape(-1, 2 * d),
                                          pc[sl][rows, idx[sl]].reshape(-1, 2 * d, 2 * d), flat(idx), T)
            cond = part if cond is None else _add_grads(part, cond, part)
    if parts is not None:
        parts["conditional"] = cond
    return _add_grads(chain, chain, cond)


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
