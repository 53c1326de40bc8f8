"""
NumPy restatement of Gaussian-process factor analysis (vidp_amd.factor_analysis_variational), two independent pieces.

1. A dense sparse-CVI model in the style of tests/np_ml.MultiLatentSparseCVI (whose dense prior, posterior and pair marginals it
   takes): the rows are the MATERIALISED projections of every output onto the pair of inducing states,
       w_ip = (W_i H) P_i [2D],   fmu_ip = w_ip . E[v],   fvar_ip = w_ip Cov[v] w_ip^T + (W_i H) T_i (W_i H)^T,
       theta_m <- (1 - lr) theta_m + lr sum_{i in m} sum_p (g1_ip w_ip, g2_ip w_ip w_ip^T),
   with H = H_1 (+) ... (+) H_L and W_i = A(t_i) B.  Nothing here passes through the L x L latent-space form of the product.
2. A dense GP log marginal with no state-space code at all: Cov(y_ip, y_jq) = sum_l W_ipl W_jql k_l(t_i - t_j) + s^2 delta,
   k_l(tau) = H_l A_l(|tau|) Pinf_l H_l^T, NaN entries dropped.

Then the sums the kernel tests compare the three entry points with, each with the sum of its absolute terms for rounding bounds.
"""
import numpy as np

from oracle import np_conditionals
from tests import np_lik, np_ml

BERNOULLI, POISSON, GAUSSIAN = 1, 2, 3          # MFGM_LIK_* of include/mfgm.h


class Gauss:
    def __init__(self, variance):
        self.v = float(variance)

    def ve_and_grads(self, mu, var, y):
        r = y - mu
        c = 0.5 * np.log(2.0 * np.pi * self.v)
        return (-c - 0.5 * (r * r + var) / self.v, r / self.v, np.full_like(mu, -0.5 / self.v),
                dict(ve=np.abs(c) + 0.5 * (r * r + np.abs(var)) / self.v, dmu=(np.abs(y) + np.abs(mu)) / self.v,
                     dv=np.full_like(mu, 0.5 / self.v)))


def make_lik(kind, param):
    return {BERNOULLI: np_lik.Bernoulli, POISSON: np_lik.Poisson, GAUSSIAN: Gauss}[kind](param)


def lik_terms(liks, fmu, fvar, Y):
    """(ve, dm, dv [N, P], dict of the sums of absolute terms of each) with likelihood liks[p] on column p; NaN observations: zeros."""
    out = [np.zeros_like(fmu) for _ in range(6)]
    for p, lk in enumerate(liks):
        seen = ~np.isnan(Y[:, p])
        e, a, b, sc = lk.ve_and_grads(fmu[seen, p], fvar[seen, p], Y[seen, p])
        for o, v in zip(out, (e, a, b, sc["ve"], sc["dmu"], sc["dv"])):
            o[seen, p] = v
    return out[0], out[1], out[2], dict(ve=out[3], dm=out[4], dv=out[5])


def weights(A, B, t):
    """W [N, P, L] = A(t) B for A an array [P, L] or a callable t -> [N, P, L]."""
    At = np.asarray(A(t) if callable(A) else np.broadcast_to(A, (len(t),) + np.shape(A)), dtype=np.float64)
    return At @ np.asarray(B, dtype=np.float64)


class FactorAnalysisSparseCVI(np_ml.MultiLatentSparseCVI):
    """kids: the oracle kernels of the L latents; z [M]; A: [P, L] or callable; B [L, L]; liks: P likelihood objects (make_lik)."""

    def __init__(self, kids, z, A, B, liks, learning_rate=0.1):
        super().__init__(kids, z, None, learning_rate)
        self.A, self.B, self.liks = A, np.asarray(B, dtype=np.float64), list(liks)
        self._rows = None

    def rows(self, t):
        """(w [N, P, 2D], conditional variances [N, P], interval [N], W [N, P, L])."""
        if self._rows is None or self._rows[0] is not t:
            Pm, T, idx = np_conditionals.conditional_statistics(t, self.z, self.kernel)
            W = weights(self.A, self.B, t)
            E = W @ self.H                                          # [N, P, D]
            self._rows = (t, E @ Pm, np.einsum("npk,nkj,npj->np", E, T, E), idx, W)
        return self._rows[1:]

    def predict_f(self, t, post=None):
        """(means, variances) [N, P]."""
        w, cv, idx, _ = self.rows(t)
        pm, pc = self.pair_marginals(post)
        fmu = np.einsum("npj,nj->np", w, pm[idx])
        fvar = cv.copy()
        for k in np.unique(idx):
            sel = idx == k
            fvar[sel] += np.einsum("npi,ij,npj->np", w[sel], pc[k], w[sel])
        return fmu, fvar

    def predict_latents(self, t):
        """(means [N, L], covariances [N, L, L]) of the latent GPs."""
        Pm, T, idx = np_conditionals.conditional_statistics(t, self.z, self.kernel)
        Hl = self.H @ Pm                                            # [N, L, 2D]
        pm, pc = self.pair_marginals()
        return np.einsum("nlj,nj->nl", Hl, pm[idx]), self.H @ T @ self.H.T + Hl @ pc[idx] @ np.swapaxes(Hl, -1, -2)

    def update_sites(self, t, Y):
        w, _, idx, _ = self.rows(t)
        mu, var = self.predict_f(t)
        _, dm, dv, _ = lik_terms(self.liks, mu, var, Y)
        g1 = dm - 2.0 * dv * mu
        s1, s2 = np.zeros_like(self.nat1), np.zeros_like(self.nat2)
        np.add.at(s1, idx, np.einsum("np,npj->nj", g1, w))
        for k in np.unique(idx):
            sel = idx == k
            s2[k] = np.einsum("np,npi,npj->ij", dv[sel], w[sel], w[sel])
        self.nat1 = (1 - self.lr) * self.nat1 + self.lr * s1
        self.nat2 = (1 - self.lr) * self.nat2 + self.lr * s2

    def elbo(self, t, Y):
        post = self.posterior()
        _, m, S, ld = post
        mu, var = self.predict_f(t, post)
        kl = 0.5 * ((self.P * S).sum() + m @ self.P @ m - m.size - self.logdetP + ld)
        return float(np.sum(lik_terms(self.liks, mu, var, Y)[0]) - kl)


def gp_log_marginal(kids, t, Y, W, noise_variance):
    """log N(y_obs; 0, C): C[(i, p), (j, q)] = sum_l W[i, p, l] W[j, q, l] k_l(t_i - t_j) + noise delta over the entries of Y [N, P]
    that are not NaN.  k_l(tau) = H_l A_l(|tau|) Pinf_l H_l^T."""
    t = np.asarray(t, dtype=np.float64)
    N, P, L = W.shape
    tau = np.abs(t[:, None] - t[None, :])
    C = np.zeros((N, P, N, P))
    for l, k in enumerate(kids):
        h = k.emission_vector()[0]
        kl = np.einsum("a,ijab,b->ij", h, k.state_transitions(tau) @ k.steady_state_covariance(), h)
        C += W[:, :, None, None, l] * W[None, None, :, :, l] * kl[:, None, :, None]
    C = C.reshape(N * P, N * P) + noise_variance * np.eye(N * P)
    y = Y.reshape(-1)
    keep = ~np.isnan(y)
    C, y = C[np.ix_(keep, keep)], y[keep]
    Lc = np.linalg.cholesky(C)
    a = np.linalg.solve(Lc, y)
    return float(-0.5 * a @ a - np.log(np.diag(Lc)).sum() - 0.5 * len(y) * np.log(2.0 * np.pi))


# ---- sums for the kernel tests -------------------------------------------------------------------------------------------------------------
def tri(L):
    """(rows, columns) of the lower triangle of an L x L matrix, row-major: the order of lcov / gam2."""
    return np.tril_indices(L)


def point_weights(W, N):
    return np.broadcast_to(W, (N,) + W.shape[-2:]) if W.ndim == 2 else W


def predict_sums(h, c, idx, pmu, pair, dl, W):
    """dict(lmu [N, L], lcov [N, LT], fmu, fvar [N, P]) and the same keys with the sums of absolute terms, from the rows h [N, 2D], the
    pair means [M + 1, 2D] and covariances, W [P, L] or [N, P, L]."""
    N, L = len(h), len(dl)
    Hl = h[:, None, :] * np_ml.slots(dl)[None]
    Wn = point_weights(W, N)
    lmu = np.einsum("nlj,nj->nl", Hl, pmu[idx])
    smu = np.einsum("nlj,nj->nl", np.abs(Hl), np.abs(pmu[idx]))
    K = np.zeros((N, L, L))
    sK = np.zeros((N, L, L))
    K[:, np.arange(L), np.arange(L)] = c
    sK[:, np.arange(L), np.arange(L)] = np.abs(c)
    for k in np.unique(idx):
        sel = idx == k
        K[sel] += np.einsum("nli,ij,nkj->nlk", Hl[sel], pair[k], Hl[sel])
        sK[sel] += np.einsum("nli,ij,nkj->nlk", np.abs(Hl[sel]), np.abs(pair[k]), np.abs(Hl[sel]))
    i, j = tri(L)
    got = dict(lmu=lmu, lcov=K[:, i, j], fmu=np.einsum("npl,nl->np", Wn, lmu), fvar=np.einsum("npl,nlk,npk->np", Wn, K, Wn))
    sc = dict(lmu=smu, lcov=sK[:, i, j], fmu=np.einsum("npl,nl->np", np.abs(Wn), smu),
              fvar=np.einsum("npl,nlk,npk->np", np.abs(Wn), sK, np.abs(Wn)))
    return got, sc


def fold(liks, fmu, fvar, Y, W):
    """The likelihood outputs at given marginals: dict(ve [N], dm, dv [N, P], gam1 [N, L], gam2 [N, LT]) and the sums of absolute
    terms under the same keys."""
    N, L = len(fmu), W.shape[-1]
    Wn = point_weights(W, N)
    ve, dm, dv, s = lik_terms(liks, fmu, fvar, Y)
    i, j = tri(L)
    g = dm - 2.0 * dv * fmu
    sg = s["dm"] + 2.0 * s["dv"] * np.abs(fmu)
    got = dict(ve=ve.sum(1), dm=dm, dv=dv, gam1=np.einsum("np,npl->nl", g, Wn), gam2=np.einsum("np,npl,npk->nlk", dv, Wn, Wn)[:, i, j])
    sc = dict(ve=s["ve"].sum(1), dm=s["dm"], dv=s["dv"], gam1=np.einsum("np,npl->nl", sg, np.abs(Wn)),
              gam2=np.einsum("np,npl,npk->nlk", s["dv"], np.abs(Wn), np.abs(Wn))[:, i, j])
    return got, sc


def site_sums(h, idx, gam1, gam2, nat1, nat2, dl, lr):
    """(nat1, nat2 dense, sums of absolute terms of each) after one update of the dense sites from gam1 [N, L], gam2 [N, LT]."""
    L = len(dl)
    lat = np.argmax(np_ml.slots(dl), axis=0)                       # the latent that owns every slot of the pair, [2D]
    i, j = tri(L)
    G = np.zeros((len(h), L, L))
    G[:, i, j] = gam2
    G[:, j, i] = gam2
    e1 = gam1[:, lat] * h
    s1, a1, s2, a2 = np.zeros_like(nat1), np.zeros_like(nat1), np.zeros_like(nat2), np.zeros_like(nat2)
    for k in np.unique(idx):
        sel = idx == k
        e2 = G[sel][:, lat][:, :, lat] * h[sel][:, :, None] * h[sel][:, None, :]
        s1[k], a1[k], s2[k], a2[k] = e1[sel].sum(0), np.abs(e1[sel]).sum(0), e2.sum(0), np.abs(e2).sum(0)
    return ((1 - lr) * nat1 + lr * s1, (1 - lr) * nat2 + lr * s2, np.abs((1 - lr) * nat1) + lr * a1, np.abs((1 - lr) * nat2) + lr * a2)


def materialised_rows(h, dl, W):
    """w [N, P, 2D] = sum_l W[i, p, l] (h_i masked to latent l): the N P scalar data points of the materialised route."""
    return np.einsum("npl,nlj->npj", point_weights(W, len(h)), h[:, None, :] * np_ml.slots(dl)[None])
