"""
Plain reference of the four tensor-product Gauss-Hermite operations of csrc/mfgm_quad.h (mfgm_quad_linearize, mfgm_quad_kl,
mfgm_quad_esde, mfgm_quad_vdp_lagrange), independent of vidp_amd: float64 NumPy and CPU torch autograd.

  * rule: numpy.polynomial.hermite.hermgauss(H) as a tensor product over d, nodes m + sqrt(2) L xi with L = chol S, weights
    prod w / pi^{d/2};
  * drifts of kinds 10 .. 15 with the parameter vectors of include/mfgm.h, as plain torch functions: every derivative (Jacobian,
    expectation parameters, drift parameters) is autograd's, through torch.linalg.cholesky -- the rule is differentiated as a formula,
    which is what the kernels' hand-written chain rule claims to do (relu'(0) = 0 in torch as in the kernel);
  * every value comes with the sum of the absolute values of its terms, from which the GPU tests build their rounding bounds.
"""
import itertools
import math

import numpy as np
import torch

EPS = 2.3e-16          # a little above the unit roundoff of fp64 per operation (tests/test_gpu_st.py)
R2 = math.sqrt(2.0)
_T = lambda x: x.transpose(-1, -2)
_t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))


def n_params(kind, nh=0):
    return 3 * nh + 1 if kind == 11 else 2


def rule(H, d, reverse=False):
    """Nodes xi [H^d, d] and weights [H^d]; the last dimension runs fastest.  reverse: the same rule visited backwards."""
    gx, gw = np.polynomial.hermite.hermgauss(H)
    xi = np.array(list(itertools.product(gx, repeat=d)))
    w = np.prod(np.array(list(itertools.product(gw, repeat=d))), axis=1) / np.pi ** (0.5 * d)
    if reverse:
        xi, w = xi[::-1].copy(), w[::-1].copy()
    return torch.from_numpy(xi), torch.from_numpy(w)


def drift(kind, th, x, nh=0):
    """f(x) for x [..., d]; th [np], or [..., np] broadcasting against x[..., 0] (one parameter vector per node)."""
    if kind == 10:
        a, tau, x1, x2 = th[..., 0], th[..., 1], x[..., 0], x[..., 1]
        return torch.stack([tau * a * (x1 - x1 ** 3 / 3.0 - x2), tau * x1 / a], dim=-1)
    if kind == 11:
        W1, b1, W2 = (th[..., None, k * nh:(k + 1) * nh] for k in range(3))
        return (W2 * torch.relu(W1 * x[..., None] + b1)).sum(-1) + th[..., 3 * nh:3 * nh + 1]
    if kind == 12:
        return th[..., 0:1] * x - th[..., 1:2] * x ** 3
    if kind == 13:
        return th[..., 0:1] * torch.tanh(x)
    if kind == 14:
        return torch.sin(x - th[..., 0:1])
    if kind == 15:
        return torch.sqrt(th[..., 0:1] * torch.abs(x))
    raise ValueError(kind)


def _nodes(m, S, H, reverse=False):
    """X [..., H^d, d] = m + sqrt(2) chol(S) xi and the weights [H^d]."""
    xi, w = rule(H, m.shape[-1], reverse)
    return m[..., None, :] + R2 * torch.einsum("...ij,hj->...hi", torch.linalg.cholesky(S), xi), w


def _sym(x):
    return 0.5 * (x + _T(x))


# ---- linearisation ------------------------------------------------------------------------------------------------------------------
def linearize(kind, th, dt, mean, cov, clip=None, nh=0):
    """A [N, d, d] = I + dt E[J], b [N, d] = dt (E f - E[J] m) on N(mean, cov) with H = 10, both clamped to clip = (lo, hi) when
    given; and the absolute sums  |I| + dt sum w |J|,  dt (sum w |f| + sum_j (sum w |J_ij|) |m_j|)  of their terms."""
    m, S, th = _t(mean), _sym(_t(cov)), _t(th)
    d = m.shape[-1]
    X, w = _nodes(m, S, 10)
    X = X.detach().requires_grad_(True)
    f = drift(kind, th, X, nh)
    J = torch.stack([torch.autograd.grad(f[..., i].sum(), X, retain_graph=True)[0] for i in range(d)], dim=-2)      # [N, M, d, d]
    f = f.detach()
    Ef, Ef_abs = torch.einsum("h,nhi->ni", w, f), torch.einsum("h,nhi->ni", w, f.abs())
    EJ, EJ_abs = torch.einsum("h,nhij->nij", w, J), torch.einsum("h,nhij->nij", w, J.abs())
    eye = torch.eye(d, dtype=torch.float64)
    A, A_abs = eye + dt * EJ, eye + dt * EJ_abs
    b = dt * (Ef - (EJ @ m[..., None])[..., 0])
    b_abs = dt * (Ef_abs + (EJ_abs @ m.abs()[..., None])[..., 0])
    A, b = A.numpy(), b.numpy()
    if clip is not None:
        A, b = np.clip(A, clip[0], clip[1]), np.clip(b, clip[0], clip[1])
    return A, b, A_abs.numpy(), b_abs.numpy()


# ---- Girsanov KL --------------------------------------------------------------------------------------------------------------------
def _kl_chain(kind, th, dt, W, logdetQp, mu0, P0, e1, ed, es, nh, reverse):
    """One chain as a differentiable function of the expectation parameters (e1 [T, d], ed [T, d, d], es [T-1, d, d]) and theta."""
    d = e1.shape[-1]
    ed = _sym(ed)
    m = e1
    S = ed - m[:, :, None] * m[:, None, :]
    C = es - m[1:, :, None] * m[:-1, None, :]
    L = torch.linalg.cholesky(S[:-1])
    A = _T(torch.cholesky_solve(_T(C), L))                                # C S^{-1}
    bq = m[1:] - (A @ m[:-1, :, None])[..., 0]
    Qq = _sym(S[1:] - A @ _T(C))
    xi, w = rule(20, d, reverse)
    X = m[:-1, None, :] + R2 * torch.einsum("tij,hj->thi", L, xi)
    r = X + dt * drift(kind, th, X, nh) - torch.einsum("tij,thj->thi", A, X) - bq[:, None, :]
    h = torch.einsum("thi,ij,thj->th", r, W, r)
    g = (h * w).sum(-1)
    ldq = 2.0 * torch.log(torch.diagonal(torch.linalg.cholesky(Qq), dim1=-2, dim2=-1)).sum(-1)
    trWQ = (W * Qq).sum(dim=(-1, -2))
    path = 0.5 * (g - d - ldq + logdetQp + trWQ).sum()
    P0inv = torch.linalg.inv(P0)
    dm = m[0] - mu0
    ld0, ldP0 = torch.linalg.slogdet(S[0])[1], torch.linalg.slogdet(P0)[1]
    kl0 = 0.5 * ((P0inv * S[0]).sum() + dm @ P0inv @ dm - d + ldP0 - ld0)
    with torch.no_grad():
        tot = 0.5 * ((h.abs() * w).sum(-1) + d + ldq.abs() + abs(logdetQp) + (W * Qq).abs().sum(dim=(-1, -2))).sum()
        tot = tot + 0.5 * ((P0inv * S[0]).abs().sum() + (dm[:, None] * P0inv * dm[None, :]).abs().sum() + d + ldP0.abs() + ld0.abs())
        # d kl / d theta_p = sum_t sum_h w dt (W r) . df/dtheta_p: the absolute sum of those terms (df/dtheta by forward mode)
        Wr, thd, tot_th = r @ W, th.detach(), []
        for p in range(th.numel()):
            e = torch.zeros_like(thd); e[p] = 1.0
            fp = torch.func.jvp(lambda v: drift(kind, v, X.detach(), nh), (thd,), (e,))[1]
            tot_th.append(float(((Wr * fp).sum(-1).abs() * w).sum() * dt))
    return path + kl0, float(tot), np.array(tot_th)


def kl(kind, th, dt, q, mu0, P0, mu, Sig, Sub, nh=0, grad=True, reverse=False):
    """KL[q || p_SDE] per chain [B] for mu [B, T, d], Sig [B, T, d, d], Sub [B, T-1, d, d] = Cov(x_{t+1}, x_t), H = 20:
        1/2 sum_t { E |x + dt f - A_t x - b_t|^2_W - d - logdet Qq_t + logdet Qp + tr(W Qq_t) } + KL[q(x0) || p(x0)],
    A_t = C_t S_t^{-1}, b_t = m_{t+1} - A_t m_t, Qq_t = S_{t+1} - A_t C_t^T, W = (dt q)^{-1}.  Returns a dict: kl [B], abs [B] (the
    absolute sum of the terms), gth_abs [B, np] (the absolute sum of the terms of d kl / d theta) and, with grad,
    g1 / gd / gs = d kl / d (eta_lin, eta_diag, eta_sub) (gd symmetric, gs = dF/dC) and gth [B, np] = d kl / d theta, all from
    torch.autograd.grad."""
    mu, Sig, Sub, th = _t(mu), _t(Sig), _t(Sub), _t(th)
    Qp = dt * _t(q)
    W, logdetQp = torch.linalg.inv(Qp), float(torch.linalg.slogdet(Qp)[1])
    mu0, P0 = _t(mu0).reshape(-1), _t(P0)
    out = dict(kl=[], abs=[], gth_abs=[], g1=[], gd=[], gs=[], gth=[])
    for b in range(mu.shape[0]):
        e1 = mu[b].clone().requires_grad_(grad)
        ed = (Sig[b] + mu[b][:, :, None] * mu[b][:, None, :]).requires_grad_(grad)
        es = (Sub[b] + mu[b][1:, :, None] * mu[b][:-1, None, :]).requires_grad_(grad)
        thb = th.clone().requires_grad_(grad)
        val, tot, tot_th = _kl_chain(kind, thb, dt, W, logdetQp, mu0, P0, e1, ed, es, nh, reverse)
        out["kl"].append(float(val.detach()))
        out["abs"].append(tot)
        out["gth_abs"].append(tot_th)
        if grad:
            g = torch.autograd.grad(val, [e1, ed, es, thb], allow_unused=True)
            g = [torch.zeros_like(x) if v is None else v for v, x in zip(g, (e1, ed, es, thb))]
            out["g1"].append(g[0].numpy()); out["gd"].append(_sym(g[1]).numpy()); out["gs"].append(g[2].numpy())
            out["gth"].append(g[3].numpy())
    return {k: np.array(v) for k, v in out.items() if len(v)}


# ---- VDP: E_sde ---------------------------------------------------------------------------------------------------------------------
def esde(kind, th, q, mean, cov, A, b, nh=0, chunk=8):
    """E [N] = 1/2 E_{N(m, S)} |f(x) + A x - b|^2_{q^-1} per node (H = 20; a sum of non-negative terms, so it is its own absolute
    sum) with autograd gradients dEdm [N, d], dEdS [N, d, d] (symmetrised), dEdA, dEdb and gth [N, np]."""
    mean, cov, A, b, th = _t(mean), _t(cov), _t(A), _t(b), _t(th)
    Wq = torch.linalg.inv(_t(q))
    res = [[] for _ in range(6)]
    for lo in range(0, mean.shape[0], chunk):
        m, S, An, bn = (x[lo:lo + chunk].clone().requires_grad_(True) for x in (mean, cov, A, b))
        thn = th.expand(m.shape[0], 1, th.numel()).clone().requires_grad_(True)
        X, w = _nodes(m, _sym(S), 20)
        r = drift(kind, thn, X, nh) + torch.einsum("nij,nhj->nhi", An, X) - bn[:, None, :]
        E = 0.5 * (torch.einsum("nhi,ij,nhj->nh", r, Wq, r) * w).sum(-1)
        g = torch.autograd.grad(E.sum(), [m, S, An, bn, thn])
        for k, v in enumerate((E.detach(), g[0], _sym(g[1]), g[2], g[3], g[4][:, 0])):
            res[k].append(v.numpy())
    return tuple(np.concatenate(r_) for r_ in res)


# ---- VDP: Lagrange sweep ------------------------------------------------------------------------------------------------------------
def vdp_lagrange(A, dEdm, dEdS, dobsm, dobsS, dt, clip=0.0):
    """The reference's backward loop, literally (`psi @ A + psi @ A`): row N - 1 is (1e-10 I, 0), then for t = N - 1 .. 1
        psi_{t-1} = psi_t - dt (psi_t A_t + psi_t A_t - dEdS_t) - dobsS_t,   lam_{t-1} = lam_t - dt (A_t lam_t - dEdm_t) - dobsm_t
    (A, dEdm, dEdS [B, N, ..], dobsm, dobsS [B, N + 1, ..]); clip > 0: NaN -> 1e-8 and clamping to [-clip, clip] of the four gradient
    arrays on load.  Returns psi, lam and the same recursion on absolute values (the absolute sums of their terms)."""
    stab = (lambda x: np.clip(np.where(np.isnan(x), 1e-8, x), -clip, clip)) if clip > 0 else (lambda x: x)
    B, N, d = dEdm.shape
    psi, lam = np.zeros((B, N, d, d)), np.zeros((B, N, d))
    psi[:, N - 1] = 1e-10 * np.eye(d)
    psi_abs, lam_abs = psi.copy(), lam.copy()
    for t in range(N - 1, 0, -1):
        P, l, At = psi[:, t], lam[:, t], A[:, t]
        gS, gm, oS, om = stab(dEdS[:, t]), stab(dEdm[:, t]), stab(dobsS[:, t]), stab(dobsm[:, t])
        psi[:, t - 1] = P - dt * (P @ At + P @ At - gS) - oS
        lam[:, t - 1] = l - dt * ((At @ l[..., None])[..., 0] - gm) - om
        Pa, la, Aa = psi_abs[:, t], lam_abs[:, t], np.abs(At)
        psi_abs[:, t - 1] = Pa + dt * (Pa @ Aa + Pa @ Aa + np.abs(gS)) + np.abs(oS)
        lam_abs[:, t - 1] = la + dt * ((Aa @ la[..., None])[..., 0] + np.abs(gm)) + np.abs(om)
    return psi, lam, psi_abs, lam_abs
