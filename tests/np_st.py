"""
Dense NumPy model of the spatio-temporal sparse CVI model (vidp_amd.spatio_temporal_variational), written from its definition with no
state-space structure: u = s(Z_s, Z_t) is one Gaussian vector of N_u = M_t Ms d_t entries (time-major, then spatial inducing point,
then state component) whose prior precision is the time kernel's dense precision repeated for every spatial inducing point; the sites
are dense [2D, 2D] blocks overlap-added into it and the posterior is one dense factorisation and inverse.

For a data point (x_i, t_i) with the pair v of inducing states around t_i (the prior's initial state pads both ends):
    a_i = chol(K_s(Z_s, Z_s))^-1 k_s(Z_s, x_i),   h_i = H_t P^t_i,   w_i[half D + j d_t + k] = a_i[j] h_i[half d_t + k]
    fmu_i = w_i^T E[v] (+ mean function),   fvar_i = w_i^T Cov[v] w_i + c_i,   c_i = k_s(x_i, x_i) - |a_i|^2 + |a_i|^2 H_t T^t_i H_t^T
and the site update is theta_m <- (1 - lr) theta_m + lr sum_{i in m} (g1_i w_i, g2_i w_i w_i^T) with the gradients taken with respect to
the expectation parameters of the centred f.  The time part (P^t, T^t, the prior precision) comes from oracle.np_kernels /
oracle.np_conditionals.
"""
import numpy as np

from oracle import np_conditionals
from tests import np_pep


def _scaled_dist2(X, X2, ls):
    A, B = np.asarray(X) / ls, np.asarray(X2) / ls
    return ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)


class SpaceKernel:
    """name in {"se", "matern12", "matern32", "matern52"}: variance k(|x - x'| / lengthscales)."""

    def __init__(self, name, lengthscales, variance):
        self.name, self.ls, self.variance = name, np.asarray(lengthscales, dtype=np.float64), float(variance)

    def K(self, X, X2=None):
        r2 = _scaled_dist2(X, X if X2 is None else X2, self.ls)
        r = np.sqrt(r2)
        if self.name == "se":
            return self.variance * np.exp(-0.5 * r2)
        if self.name == "matern12":
            return self.variance * np.exp(-r)
        if self.name == "matern32":
            return self.variance * (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
        return self.variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * np.exp(-np.sqrt(5.0) * r)


def features(ks, kt, Zs, z, X):
    """(a [N, Ms], h [N, 2 d_t], c [N], interval [N]) of the inputs X [N, p + 1] (time last)."""
    x, t = X[:, :-1], X[:, -1]
    L = np.linalg.cholesky(ks.K(Zs))
    a = np.linalg.solve(L, ks.K(Zs, x)).T
    P, T, idx = np_conditionals.conditional_statistics(t, np.asarray(z, dtype=np.float64), kt)
    Ht = kt.emission_vector()[0]
    h = np.einsum("k,nkl->nl", Ht, P)
    ct = np.einsum("k,nkl,l->n", Ht, T, Ht)
    a2 = (a * a).sum(-1)
    return a, h, ks.variance - a2 + a2 * ct, idx


def kron_w(a, h):
    N, Ms = a.shape
    dt = h.shape[1] // 2
    return (a[:, None, :, None] * h.reshape(N, 2, 1, dt)).reshape(N, 2 * Ms * dt)


def _inv_logdet(A):
    """(A^-1, log det A) of a symmetric positive definite matrix by one Cholesky factorisation."""
    try:
        from scipy.linalg import lapack
        c, info = lapack.dpotrf(A, lower=1)
        assert info == 0
        ld = 2.0 * np.log(np.diag(c)).sum()
        inv, info = lapack.dpotri(c, lower=1)
        assert info == 0
        inv = np.tril(inv)
        return inv + np.tril(inv, -1).T, ld
    except ImportError:
        return np.linalg.inv(A), np.linalg.slogdet(A)[1]


class SpatioTemporalSparseCVI:
    def __init__(self, Zs, z, ks, kt, lik, mean_function=None, learning_rate=0.1):
        self.Zs, self.z, self.ks, self.kt, self.lik = np.asarray(Zs, dtype=np.float64), np.asarray(z, dtype=np.float64), ks, kt, lik
        self.mean_function, self.lr = mean_function, learning_rate
        self.Ms, self.dt, self.M = self.Zs.shape[0], kt.state_dim, self.z.shape[0]
        self.D = self.Ms * self.dt
        self.nat1 = np.zeros((self.M + 1, 2 * self.D))
        self.nat2 = np.zeros((self.M + 1, 2 * self.D, 2 * self.D))
        M, Ms, dt, D = self.M, self.Ms, self.dt, self.D
        Pt = np_pep.dense_precision(kt.state_space_model(self.z)).reshape(M, dt, M, dt)
        P = np.zeros((M, Ms, dt, M, Ms, dt))
        for j in range(Ms):
            P[:, j, :, :, j, :] = Pt
        self.P = P.reshape(M * D, M * D)
        self.logdetP = np.linalg.slogdet(self.P)[1]
        P0t = kt.steady_state_covariance() + kt.jitter * np.eye(dt)
        self.P0 = np.kron(np.eye(Ms), P0t)
        self._feat = None

    def _features(self, X):
        if self._feat is None or self._feat[0] is not X:
            a, h, c, idx = features(self.ks, self.kt, self.Zs, self.z, X)
            self._feat = (X, kron_w(a, h), c, idx)
        return self._feat[1:]

    def posterior(self):
        """(precision, mean, covariance, log det precision) of q(u)."""
        c = getattr(self, "_post", None)
        if c is not None and c[0] is self.nat1 and c[1] is self.nat2:          # update_sites replaces both arrays
            return c[2]
        M, D = self.M, self.D
        b = np.zeros((M + 2) * D)
        Q = np.zeros(((M + 2) * D, (M + 2) * D))
        for m in range(M + 1):
            sl = slice(m * D, (m + 2) * D)
            b[sl] += self.nat1[m]
            Q[sl, sl] += -2.0 * self.nat2[m]
        Lam = self.P + Q[D:-D, D:-D]
        S, ld = _inv_logdet(Lam)
        self._post = (self.nat1, self.nat2, (Lam, S @ b[D:-D], S, ld))
        return self._post[2]

    def pair_marginals(self, post=None):
        M, D = self.M, self.D
        _, m, S, _ = self.posterior() if post is None else post
        mu = np.concatenate([np.zeros((1, D)), m.reshape(M, D), np.zeros((1, D))])
        blk = S.reshape(M, D, M, D)
        pm = np.concatenate([mu[:-1], mu[1:]], axis=-1)
        pc = np.zeros((M + 1, 2 * D, 2 * D))
        for k in range(M + 1):
            pc[k, :D, :D] = self.P0 if k == 0 else blk[k - 1, :, k - 1, :]
            pc[k, D:, D:] = self.P0 if k == M else blk[k, :, k, :]
            if 0 < k < M:
                pc[k, D:, :D] = blk[k, :, k - 1, :]
                pc[k, :D, D:] = blk[k, :, k - 1, :].T
        return pm, pc

    def predict_f(self, X, post=None):
        """(mean, variance) [N, 1], the mean function included."""
        w, c, idx = self._features(X)
        pm, pc = self.pair_marginals(post)
        fmu = (w * pm[idx]).sum(-1)
        fvar = c.copy()
        for k in np.unique(idx):          # per interval: no [N, 2D, 2D] gather
            sel = idx == k
            fvar[sel] += np.einsum("ni,ij,nj->n", w[sel], pc[k], w[sel])
        if self.mean_function is not None:
            fmu = fmu + self.mean_function(X)[:, 0]
        return fmu[:, None], fvar[:, None]

    def update_sites(self, X, y):
        w, _, idx = self._features(X)
        mu, var = self.predict_f(X)
        g1, g2 = self.lik.grads_expectation(mu, var, y)
        if self.mean_function is not None:
            g1 = g1 + 2.0 * g2 * self.mean_function(X)
        s1, s2 = np.zeros_like(self.nat1), np.zeros_like(self.nat2)
        np.add.at(s1, idx, g1 * w)
        for k in np.unique(idx):
            sel = idx == k
            s2[k] = np.einsum("n,ni,nj->ij", g2[sel, 0], w[sel], w[sel])
        self.nat1 = (1 - self.lr) * self.nat1 + self.lr * s1
        self.nat2 = (1 - self.lr) * self.nat2 + self.lr * s2

    def elbo(self, X, y):
        post = self.posterior()
        _, m, S, ld = post
        mu, var = self.predict_f(X, post)
        kl = 0.5 * ((self.P * S).sum() + m @ self.P @ m - m.size - self.logdetP + ld)
        return float(np.sum(self.lik.variational_expectations(mu, var, y)) - kl)

    def predict_log_density(self, X, y):
        return self.lik.predict_log_density(*self.predict_f(X), y)


def gpr(ks, kt_cov, X, y, noise, mean=None):
    """Dense GP regression with k((x, t), (x', t')) = k_s(x, x') k_t(t - t'): (log marginal likelihood, posterior mean [N] at X)."""
    K = ks.K(X[:, :-1]) * kt_cov(X[:, -1][:, None] - X[:, -1][None, :])
    r = y.reshape(-1) - (0.0 if mean is None else mean(X)[:, 0])
    L = np.linalg.cholesky(K + noise * np.eye(len(r)))
    al = np.linalg.solve(L.T, np.linalg.solve(L, r))
    lml = -0.5 * r @ al - np.log(np.diag(L)).sum() - 0.5 * len(r) * np.log(2.0 * np.pi)
    return float(lml), K @ al + (0.0 if mean is None else mean(X)[:, 0])
