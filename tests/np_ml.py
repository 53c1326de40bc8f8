"""
Dense NumPy model of the multi-latent sparse CVI model (vidp_amd.multi_latent_variational), written from its definition with no
state-space structure and no block structure: u = s(Z) is one Gaussian vector of M D entries (time-major) with the stacked kernel's
dense prior precision; the projections are materialised rows W [N, L, 2D] = H P_i (row l for latent l), the sites are dense [2D, 2D]
blocks overlap-added into the precision, the posterior is one dense factorisation and inverse.

    fmu[i, l] = W[i, l] . E[v],   fvar[i, l] = W[i, l] Cov[v] W[i, l]^T + (H T_i H^T)[l, l]          v: the pair of states around t_i
    theta_m <- (1 - lr) theta_m + lr sum_{i in m} sum_l (g1[i, l] W[i, l], g2[i, l] W[i, l] W[i, l]^T)

The likelihoods restate the rule through tests/np_lik.py (Bernoulli terms of MultiStage) and the closed forms (Poisson term,
heteroskedastic Gaussian); every method also returns the sum of the absolute terms of what it sums, for rounding bounds.
"""
import numpy as np

from oracle import np_conditionals, np_kernels
from tests import np_lik, np_pep
from tests.np_st import _inv_logdet


class MultiStage:
    latent_dim = 3

    def __init__(self, jitter=1e-3, binsize=1.0):
        self.bern, self.pois = np_lik.Bernoulli(jitter), np_lik.Poisson(binsize)

    def ve_and_derivatives(self, mu, var, y):
        """(VE [N], dVE/dm [N, 3], dVE/dv [N, 3], dict of the sums of absolute terms of each); y [N]."""
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        with np.errstate(invalid="ignore"):
            is0, is1, big = y == 0, y == 1, y >= 2
        in0, in1 = is0 | is1 | big, is1 | big
        N = len(y)
        ve, dm, dv = np.zeros(N), np.zeros((N, 3)), np.zeros((N, 3))
        sve, sdm, sdv = np.zeros(N), np.zeros((N, 3)), np.zeros((N, 3))
        for l, (sel, lab) in enumerate(((in0, is0), (in1, is1))):
            e, a, b, sc = self.bern.ve_and_grads(mu[sel, l], var[sel, l], lab[sel].astype(np.float64))
            ve[sel] += e
            sve[sel] += sc["ve"]
            dm[sel, l], dv[sel, l], sdm[sel, l], sdv[sel, l] = a, b, sc["dmu"], sc["dv"]
        e, a, b, sc = self.pois.ve_and_grads(mu[big, 2], var[big, 2], y[big] - 2.0)
        ve[big] += e
        sve[big] += sc["ve"]
        dm[big, 2], dv[big, 2], sdm[big, 2], sdv[big, 2] = a, b, sc["dmu"], sc["dv"]
        return ve, dm, dv, dict(ve=sve, dm=sdm, dv=sdv)

    def log_prob(self, F, y):
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        with np.errstate(invalid="ignore"):
            is0, is1, big = y == 0, y == 1, y >= 2
        lp = lambda f: np.log(self.bern.p(f))
        out = np.zeros(len(y))
        out[is0] = lp(F[is0, 0])
        out[is1] = lp(-F[is1, 0]) + lp(F[is1, 1])
        out[big] = lp(-F[big, 0]) + lp(-F[big, 1]) + self.pois.log_prob(F[big, 2], y[big] - 2.0)
        return out


class HetGauss:
    latent_dim = 2

    def ve_and_derivatives(self, mu, var, y):
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        m0, m1, v0, v1 = mu[:, 0], mu[:, 1], var[:, 0], var[:, 1]
        s = np.exp(-m1 + 0.5 * v1)
        r = m0 - y
        q = r * r + v0
        ve = -0.5 * (np.log(2.0 * np.pi) + m1 + s * q)
        dm = np.stack([-s * r, -0.5 + 0.5 * s * q], -1)
        dv = np.stack([-0.5 * s, -0.25 * s * q], -1)
        return ve, dm, dv, dict(ve=0.5 * (np.log(2.0 * np.pi) + np.abs(m1) + s * q), dm=np.stack([s * np.abs(r), 0.5 + 0.5 * s * q], -1),
                                dv=np.abs(dv))

    def log_prob(self, F, y):
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        return -0.5 * (np.log(2.0 * np.pi) + F[:, 1] + np.exp(-F[:, 1]) * (y - F[:, 0]) ** 2)


def grads_expectation(lik, mu, var, y):
    """(VE, g1, g2, sums of absolute terms): g1 = dm - 2 dv m, g2 = dv."""
    ve, dm, dv, sc = lik.ve_and_derivatives(mu, var, y)
    return ve, dm - 2.0 * dv * mu, dv, dict(ve=sc["ve"], g1=sc["dm"] + 2.0 * sc["dv"] * np.abs(mu), g2=sc["dv"])


def emission(kids):
    """[L, D]: row l holds child l's emission row at child l's slice of the stacked state."""
    D = sum(k.state_dim for k in kids)
    H = np.zeros((len(kids), D))
    o = 0
    for l, k in enumerate(kids):
        H[l, o:o + k.state_dim] = k.emission_vector()[0]
        o += k.state_dim
    return H


class MultiLatentSparseCVI:
    """kids: the oracle kernels (oracle.np_kernels) of the L latents; z [M]; lik: MultiStage or HetGauss above."""

    def __init__(self, kids, z, lik, learning_rate=0.1):
        self.kids, self.z, self.lik, self.lr = list(kids), np.asarray(z, dtype=np.float64), lik, learning_rate
        self.kernel = np_kernels.Sum(self.kids)
        self.H = emission(self.kids)
        self.L, self.D, self.M = len(self.kids), self.kernel.state_dim, len(self.z)
        self.nat1 = np.zeros((self.M + 1, 2 * self.D))
        self.nat2 = np.zeros((self.M + 1, 2 * self.D, 2 * self.D))
        self.P = np_pep.dense_precision(self.kernel.state_space_model(self.z))
        self.logdetP = np.linalg.slogdet(self.P)[1]
        self.P0 = self.kernel.steady_state_covariance() + self.kernel.jitter * np.eye(self.D)
        self._feat = None

    def features(self, t):
        """(W [N, L, 2D], c [N, L], interval [N])."""
        if self._feat is None or self._feat[0] is not t:
            P, T, idx = np_conditionals.conditional_statistics(t, self.z, self.kernel)
            W = np.einsum("lk,nkj->nlj", self.H, P)
            c = np.einsum("lk,nkj,lj->nl", self.H, T, self.H)
            self._feat = (t, W, c, idx)
        return self._feat[1:]

    def posterior(self):
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

    def predict_f(self, t, post=None):
        """(means, variances) [N, L]."""
        W, c, idx = self.features(t)
        pm, pc = self.pair_marginals(post)
        fmu = np.einsum("nlj,nj->nl", W, pm[idx])
        fvar = c.copy()
        for k in np.unique(idx):
            sel = idx == k
            fvar[sel] += np.einsum("nli,ij,nlj->nl", W[sel], pc[k], W[sel])
        return fmu, fvar

    def update_sites(self, t, y):
        W, _, idx = self.features(t)
        mu, var = self.predict_f(t)
        _, g1, g2, _ = grads_expectation(self.lik, mu, var, y)
        s1, s2 = np.zeros_like(self.nat1), np.zeros_like(self.nat2)
        np.add.at(s1, idx, np.einsum("nl,nlj->nj", g1, W))
        for k in np.unique(idx):
            sel = idx == k
            s2[k] = np.einsum("nl,nli,nlj->ij", g2[sel], W[sel], W[sel])
        self.nat1 = (1 - self.lr) * self.nat1 + self.lr * s1
        self.nat2 = (1 - self.lr) * self.nat2 + self.lr * s2

    def elbo(self, t, y):
        post = self.posterior()
        _, m, S, ld = post
        mu, var = self.predict_f(t, post)
        kl = 0.5 * ((self.P * S).sum() + m @ self.P @ m - m.size - self.logdetP + ld)
        return float(np.sum(self.lik.ve_and_derivatives(mu, var, y)[0]) - kl)


# ---- seeded data of the model tests ---------------------------------------------------------------------------------------------------------
def multistage_data(rng, z, N):
    """Sorted times over the inducing grid (a little beyond both ends) and counts drawn down the tree from smooth latents; y [N, 1]."""
    from scipy import special
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=N))
    p0 = 0.5 * special.erfc(-(0.8 * np.sin(0.9 * t)) / np.sqrt(2.0))
    p1 = 0.5 * special.erfc(-(0.6 * np.cos(0.5 * t)) / np.sqrt(2.0))
    lam = np.exp(0.4 * np.sin(0.3 * t) + 0.2)
    e0, e1 = rng.uniform(size=N) < p0, rng.uniform(size=N) < p1
    y = np.where(e0, 0.0, np.where(e1, 1.0, 2.0 + rng.poisson(lam)))
    return t, y[:, None]


def hetgauss_data(rng, z, N):
    """Sorted times and y = sin(0.8 t) + noise whose log-variance is 0.6 cos(0.4 t) - 1; y [N, 1]."""
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=N))
    y = np.sin(0.8 * t) + np.exp(0.5 * (0.6 * np.cos(0.4 * t) - 1.0)) * rng.normal(size=N)
    return t, y[:, None]


# ---- sums for the kernel tests -------------------------------------------------------------------------------------------------------------
def slots(dl):
    """[L, 2D] 0/1: the slots of the pair that latent l owns."""
    D = sum(dl)
    mask = np.zeros((len(dl), 2 * D))
    o = 0
    for l, n in enumerate(dl):
        mask[l, o:o + n] = mask[l, D + o:D + o + n] = 1.0
        o += n
    return mask


def predict_sums(h, c, idx, pmu, pair, dl):
    """(fmu, fvar [N, L], sums of absolute terms of each) from the rows h [N, 2D], the pair means [M + 1, 2D] and covariances."""
    W = h[:, None, :] * slots(dl)[None]
    fmu = np.einsum("nlj,nj->nl", W, pmu[idx])
    smu = np.einsum("nlj,nj->nl", np.abs(W), np.abs(pmu[idx]))
    fvar, svar = c.copy(), np.abs(c)
    for k in np.unique(idx):
        sel = idx == k
        fvar[sel] += np.einsum("nli,ij,nlj->nl", W[sel], pair[k], W[sel])
        svar[sel] += np.einsum("nli,ij,nlj->nl", np.abs(W[sel]), np.abs(pair[k]), np.abs(W[sel]))
    return fmu, fvar, smu, svar


def site_sums(h, idx, g1, g2, nat1, nat2, dl, lr):
    """(nat1, nat2 dense, sums of absolute terms of each) after one update of the dense sites."""
    W = h[:, None, :] * slots(dl)[None]
    s1, a1 = np.zeros_like(nat1), np.zeros_like(nat1)
    np.add.at(s1, idx, np.einsum("nl,nlj->nj", g1, W))
    np.add.at(a1, idx, np.einsum("nl,nlj->nj", np.abs(g1), np.abs(W)))
    s2, a2 = np.zeros_like(nat2), np.zeros_like(nat2)
    for k in np.unique(idx):
        sel = idx == k
        s2[k] = np.einsum("nl,nli,nlj->ij", g2[sel], W[sel], W[sel])
        a2[k] = np.einsum("nl,nli,nlj->ij", np.abs(g2[sel]), np.abs(W[sel]), np.abs(W[sel]))
    return ((1 - lr) * nat1 + lr * s1, (1 - lr) * nat2 + lr * s2, np.abs((1 - lr) * nat1) + lr * a1, np.abs((1 - lr) * nat2) + lr * a2)
