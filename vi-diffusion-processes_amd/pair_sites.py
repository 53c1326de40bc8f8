"""
What the models with sites on pairs of consecutive inducing states share (SparseCVIGaussianProcess and the models built on it in
sparse_pep.py, spatio_temporal_variational.py, multi_latent_variational.py, factor_analysis_variational.py, and PanelSparseCVI): the
CPU correctness anchor -- a dense precision over all inducing states, its posterior for given sites, the pair marginals and the KL term
-- and the small per-data-set helpers of the device routes.  A `model` here is anything with `_kernel`, `inducing_inputs` [M], sites
`nat1` [..., M + 1, 2d] / `nat2` [..., M + 1, 2d, 2d] and the `_key()` / `_current()` stamps of its sites; every function takes an
optional leading batch axis on the sites (the series of a panel), so one chain and B chains run the same code.
"""
import torch

from .conditionals import pair_moments


def on_device(model):
    return model.inducing_inputs.is_cuda


def need_device(model, what):
    if not on_device(model):
        raise NotImplementedError(f"{what} needs the model on the device; CPU tensors serve the torch route of small models only")


# ---- the dense anchor (CPU tensors: small models, the host tests) ------------------------------------------------------------------------
def dense_prior(model):
    """dict(P: the prior precision over all inducing states as one dense [Md, Md] matrix, logdet: its log determinant); cached, the
    prior is fixed."""
    c = getattr(model, "_dense_p", None)
    if c is None:
        z, kernel = model.inducing_inputs, model._kernel
        M, d = z.shape[0], kernel.state_dim
        A, Q = kernel.transition_statistics_local(z[1:] - z[:-1])
        Qi = torch.linalg.inv(Q)
        P = torch.zeros((M * d, M * d), dtype=torch.float64)
        P[:d, :d] = torch.linalg.inv(kernel.initial_covariance_matrix())
        for t in range(M - 1):
            lo, hi = slice(t * d, (t + 1) * d), slice((t + 1) * d, (t + 2) * d)
            QA = Qi[t] @ A[t]
            P[lo, lo] += A[t].T @ QA
            P[hi, hi] += Qi[t]
            P[hi, lo] -= QA
            P[lo, hi] -= QA.T
        c = model._dense_p = dict(P=P, logdet=torch.linalg.slogdet(P)[1])
    return c


def dense_posterior(model, nat1=None, nat2=None):
    """(Lambda_q [..., Md, Md], mu_q [..., Md], Sigma_q [..., Md, Md]) with the sites overlap-added densely: the model's own sites
    (cached until they move) or the given ones."""
    own = nat1 is None and nat2 is None
    c = getattr(model, "_dense_q", None)
    if own and c is not None and model._current(c[0]):
        return c[1]
    nat1 = model.nat1 if nat1 is None else nat1
    nat2 = model.nat2 if nat2 is None else nat2
    lead, M1, d = nat1.shape[:-2], nat1.shape[-2], nat1.shape[-1] // 2
    b = torch.zeros(lead + ((M1 + 1) * d,), dtype=torch.float64)
    Q = torch.zeros(lead + ((M1 + 1) * d, (M1 + 1) * d), dtype=torch.float64)
    for m in range(M1):
        sl = slice(m * d, (m + 2) * d)
        b[..., sl] += nat1[..., m, :]
        Q[..., sl, sl] += -2.0 * nat2[..., m, :, :]
    P = dense_prior(model)["P"] + Q[..., d:-d, d:-d]
    S = torch.linalg.inv(P)
    val = (P, (S @ b[..., d:-d, None])[..., 0] if lead else S @ b[d:-d], S)
    if own:
        model._dense_q = (model._key(), val)
    return val


def pair_marginals(model, blocks=None):
    """Means [..., M + 1, 2d] and covariances [..., M + 1, 2d, 2d] of the pairs of consecutive inducing states, the prior's initial
    state at both ends (conditionals.py:424-470).  blocks: (mu [..., M, d], Sig [..., M, d, d], Sub [..., M - 1, d, d]) of the
    posterior from the device sweeps; None: those of the dense posterior."""
    kernel = model._kernel
    if blocks is None:
        _, mq, S = dense_posterior(model)
        d = kernel.state_dim
        lead, M = mq.shape[:-1], mq.shape[-1] // d
        blk, ar = S.view(lead + (M, d, M, d)), torch.arange(M)
        # (two index tensors apart: their axis comes out first)
        blocks = mq.view(lead + (M, d)), blk[..., ar, :, ar, :].movedim(0, -3), blk[..., ar[1:], :, ar[:-1], :].movedim(0, -3)
    mu, Sig, Sub = blocks
    return pair_moments(mu, Sig, Sub, kernel.initial_mean(()).to(mu.device, torch.float64),
                        kernel.initial_covariance_matrix().to(mu.device, torch.float64))


def dense_kl(model):
    """KL[q(s_Z) || p(s_Z)] of every chain from the dense posterior, [...]."""
    pr = dense_prior(model)
    P, mq, S = dense_posterior(model)
    if mq.dim() == 1:
        tr, mh = (pr["P"] * S).sum(), mq @ pr["P"] @ mq
    else:
        tr, mh = (pr["P"] * S).sum((-1, -2)), torch.einsum("bi,ij,bj->b", mq, pr["P"], mq)
    return 0.5 * (tr + mh - mq.shape[-1] - pr["logdet"] + torch.linalg.slogdet(P)[1])


def chain_kl(p, marginals, prior_natural, prior_mean):
    """The same KL of every chain on the device, [B]: from the packed marginal blocks of q (a model's _marginals()) and the prior's
    packed naturals (state_space_model.py:528-593)."""
    s, nat = marginals["packed"], prior_natural["nat"]
    tr, mh = p.plan.kl_terms(s["Sig"], s["Sub"], s["x"], nat["diag"], nat["sub"], prior_mean, aD=-2.0, aS=-1.0)
    return 0.5 * (tr + mh - float(p.T * p.d) + 2.0 * nat["sumlogchol"] + 2.0 * marginals["logdetL"])


# ---- per-data-set helpers of the device routes ---------------------------------------------------------------------------------------------
def csr_offsets(idx, n):
    """int32 CSR offsets [..., n + 1] of sorted data points from their interval index idx [..., N] in 0 .. n - 1."""
    cnt = torch.zeros(idx.shape[:-1] + (n,), dtype=torch.int64, device=idx.device).scatter_add_(-1, idx, torch.ones_like(idx))
    seg = torch.zeros(idx.shape[:-1] + (n + 1,), dtype=torch.int32, device=idx.device)
    seg[..., 1:] = torch.cumsum(cnt, -1).to(torch.int32)
    return seg


def initial_state(kernel, z):
    """The prior's initial mean [d] and covariance [d, d] (at the first inducing point) as contiguous fp64 tensors on z's device."""
    return (kernel.initial_mean(()).to(z.device, torch.float64).contiguous(),
            kernel.initial_covariance(z[:1]).to(z.device, torch.float64).contiguous())


def slot_mask(dl, device):
    """[L, 2D]: the slots of a pair of stacked states (D = sum dl, latent l in off_l .. off_l + dl[l]) that latent l owns."""
    D = sum(dl)
    mask = torch.zeros((len(dl), 2 * D), dtype=torch.float64)
    o = 0
    for l, n in enumerate(dl):
        mask[l, o:o + n] = 1.0
        mask[l, D + o:D + o + n] = 1.0
        o += n
    return mask.to(device)
