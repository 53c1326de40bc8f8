"""
NumPy restatement of the panel sparse CVI model (vidp_amd.panel_variational_cvi.PanelSparseCVI) and of its three kernels
(csrc/mfgm_panel.h).

The model: `SeriesSparseCVI` is the dense model of ONE series written from its definition -- u = s(Z) one Gaussian vector of M d entries
with the kernel's dense prior precision, the sites dense [2d, 2d] blocks overlap-added into it, one dense inverse -- and `Panel` loops
it over the B rows, handing every series its non-NaN points only (an absent point is simply not there).

The kernels: sums for mfgm_panel_theta / mfgm_panel_predict_lik / mfgm_panel_site_update together with the sums of the absolute terms
(for rounding bounds), and the packed layout of a B-chain plan restated from its definition (`packed_offsets`, `pack`): node t of chain
b lives in lane b P + t // R at step t % R, element e of it at (((lane // 64) R + step) E + e) 64 + lane % 64.
"""
import numpy as np

from oracle import np_conditionals
from tests import np_lik, np_pep
from tests.np_st import _inv_logdet


class Gaussian:
    def __init__(self, variance):
        self.v = float(variance)

    def ve_and_grads(self, mu, var, y):
        v, r = self.v, y - mu
        ve = -0.5 * np.log(2.0 * np.pi * v) - 0.5 * (r * r + var) / v
        dv = np.full_like(mu, -0.5 / v)
        return ve, r / v, dv, dict(ve=0.5 * np.abs(np.log(2.0 * np.pi * v)) + 0.5 * (r * r + np.abs(var)) / v, dmu=np.abs(r) / v,
                                   dv=np.abs(dv))


def likelihood(kind, param):
    """kind: 'gaussian' (param = variance), 'bernoulli' (jitter), 'poisson' (bin size)."""
    return {"gaussian": Gaussian, "bernoulli": np_lik.Bernoulli, "poisson": np_lik.Poisson}[kind](param)


def lik_terms(lik, mu, var, y):
    """(VE, g1, g2, sums of absolute terms of each) per point; a NaN observation gives exact zeros (and zero scales)."""
    mu, var, y = (np.asarray(a, dtype=np.float64) for a in (mu, var, y))
    ok = ~np.isnan(y)
    ve, g1, g2 = np.zeros_like(mu), np.zeros_like(mu), np.zeros_like(mu)
    sc = dict(ve=np.zeros_like(mu), g1=np.zeros_like(mu), g2=np.zeros_like(mu))
    if ok.any():
        e, dm, dv, s = lik.ve_and_grads(mu[ok], var[ok], y[ok])
        ve[ok], g1[ok], g2[ok] = e, dm - 2.0 * dv * mu[ok], dv
        sc["ve"][ok], sc["g1"][ok], sc["g2"][ok] = s["ve"], s["dmu"] + 2.0 * s["dv"] * np.abs(mu[ok]), s["dv"]
    return ve, g1, g2, sc


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
class SeriesSparseCVI:
    """One series: kernel (oracle.np_kernels), inducing points z [M], a likelihood with ve_and_grads."""

    def __init__(self, kernel, z, lik, learning_rate=0.1):
        self.kernel, self.z, self.lik, self.lr = kernel, np.asarray(z, dtype=np.float64), lik, learning_rate
        self.d, self.M = kernel.state_dim, len(self.z)
        self.h = np.asarray(kernel.emission_vector(), dtype=np.float64).reshape(-1)
        self.nat1 = np.zeros((self.M + 1, 2 * self.d))
        self.nat2 = np.zeros((self.M + 1, 2 * self.d, 2 * self.d))
        self.P = np_pep.dense_precision(kernel.state_space_model(self.z))
        self.logdetP = np.linalg.slogdet(self.P)[1]
        self.P0 = kernel.steady_state_covariance() + kernel.jitter * np.eye(self.d)
        self.m0 = np.asarray(kernel.initial_mean(), dtype=np.float64).reshape(-1)

    def features(self, t):
        """(w [n, 2d], c [n], interval [n])."""
        t = np.asarray(t, dtype=np.float64)
        if len(t) == 0:
            return np.zeros((0, 2 * self.d)), np.zeros(0), np.zeros(0, dtype=np.int64)
        P, T, idx = np_conditionals.conditional_statistics(t, self.z, self.kernel)
        return np.einsum("k,nkj->nj", self.h, P), np.einsum("k,nkj,j->n", self.h, T, self.h), idx

    def posterior(self):
        M, d = self.M, self.d
        b = np.zeros((M + 2) * d)
        Q = np.zeros(((M + 2) * d, (M + 2) * d))
        for m in range(M + 1):
            sl = slice(m * d, (m + 2) * d)
            b[sl] += self.nat1[m]
            Q[sl, sl] += -2.0 * self.nat2[m]
        Lam = self.P + Q[d:-d, d:-d]
        S, ld = _inv_logdet(Lam)
        return Lam, S @ b[d:-d], S, ld

    def pair_marginals(self, post):
        M, d = self.M, self.d
        _, m, S, _ = post
        mu = np.concatenate([self.m0[None], m.reshape(M, d), self.m0[None]])
        blk = S.reshape(M, d, M, d)
        pm = np.concatenate([mu[:-1], mu[1:]], axis=-1)
        pc = np.zeros((M + 1, 2 * d, 2 * d))
        for k in range(M + 1):
            pc[k, :d, :d] = self.P0 if k == 0 else blk[k - 1, :, k - 1, :]
            pc[k, d:, d:] = self.P0 if k == M else blk[k, :, k, :]
            if 0 < k < M:
                pc[k, d:, :d] = blk[k, :, k - 1, :]
                pc[k, :d, d:] = blk[k, :, k - 1, :].T
        return pm, pc

    def predict_f(self, t, post=None):
        w, c, idx = self.features(t)
        pm, pc = self.pair_marginals(self.posterior() if post is None else post)
        return np.einsum("nj,nj->n", w, pm[idx]), c + np.einsum("ni,nij,nj->n", w, pc[idx], w)

    def update_sites(self, t, y):
        w, _, idx = self.features(t)
        mu, var = self.predict_f(t)
        _, g1, g2, _ = lik_terms(self.lik, mu, var, y)
        s1, s2 = np.zeros_like(self.nat1), np.zeros_like(self.nat2)
        np.add.at(s1, idx, g1[:, None] * w)
        np.add.at(s2, idx, g2[:, None, None] * w[:, :, None] * w[:, None, :])
        self.nat1 = (1 - self.lr) * self.nat1 + self.lr * s1
        self.nat2 = (1 - self.lr) * self.nat2 + self.lr * s2

    def kl(self, post):
        _, m, S, ld = post
        return 0.5 * ((self.P * S).sum() + m @ self.P @ m - m.size - self.logdetP + ld)

    def elbo(self, t, y):
        post = self.posterior()
        mu, var = self.predict_f(t, post)
        return float(np.sum(lik_terms(self.lik, mu, var, y)[0]) - self.kl(post))


class Panel:
    """B series looped: t [B, N], y [B, N] with NaN for absent points; every series sees its present points only."""

    def __init__(self, kernel, z, lik, num_series, learning_rate=0.1):
        self.series = [SeriesSparseCVI(kernel, z, lik, learning_rate) for _ in range(num_series)]

    @staticmethod
    def _rows(t, y):
        y = np.asarray(y, dtype=np.float64).reshape(np.shape(t))
        for tb, yb in zip(np.asarray(t, dtype=np.float64), y):
            ok = ~np.isnan(yb)
            yield tb[ok], yb[ok]

    def update_sites(self, t, y):
        for s, (tb, yb) in zip(self.series, self._rows(t, y)):
            s.update_sites(tb, yb)

    def elbo_per_series(self, t, y):
        return np.array([s.elbo(tb, yb) for s, (tb, yb) in zip(self.series, self._rows(t, y))])

    def predict_f(self, t):
        out = [s.predict_f(tb) for s, tb in zip(self.series, np.asarray(t, dtype=np.float64))]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    @property
    def nat1(self):
        return np.stack([s.nat1 for s in self.series])

    @property
    def nat2(self):
        return np.stack([s.nat2 for s in self.series])


def panel_data(rng, kind, z, B, N, absent=0.15):
    """Sorted times per row over the inducing grid (a little beyond both ends), observations of the kind, about `absent` of them NaN;
    (t [B, N], y [B, N, 1])."""
    from scipy import special
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=(B, N)), axis=1)
    f = 0.8 * np.sin(0.9 * t + rng.uniform(0, 6, size=(B, 1)))
    if kind == "gaussian":
        y = f + 0.3 * rng.normal(size=t.shape)
    elif kind == "bernoulli":
        y = (rng.uniform(size=t.shape) < 0.5 * special.erfc(-f / np.sqrt(2.0))).astype(np.float64)
    else:
        y = rng.poisson(np.exp(f + 0.2)).astype(np.float64)
    y[rng.uniform(size=t.shape) < absent] = np.nan
    return t, y[..., None]


# ---- the packed layout ----------------------------------------------------------------------------------------------------------------------
def n_elems(kind, d):
    """Doubles per node: kind 0 vector, 1 full block (row-major), 2 symmetric block (lower triangle, row-major)."""
    return d if kind == 0 else (d * d if kind == 1 else d * (d + 1) // 2)


def packed_offsets(B, T, R, P, E):
    """[B, T, E] offsets of every element in the packed array."""
    b, t, e = np.meshgrid(np.arange(B), np.arange(T), np.arange(E), indexing="ij")
    lane, step = b * P + t // R, t % R
    return (((lane // 64) * R + step) * E + e) * 64 + lane % 64


def pack(kind, natural, R, P, size):
    """natural [B, n, d] or [B, n, d, d] -> the packed array of `size` doubles (zeros elsewhere)."""
    B, n, d = natural.shape[:3]
    if kind == 0:
        vals = natural
    elif kind == 1:
        vals = natural.reshape(B, n, d * d)
    else:
        i, j = np.tril_indices(d)
        vals = natural[:, :, i, j]
    out = np.zeros(size)
    if n > 0:
        out[packed_offsets(B, n, R, P, vals.shape[-1])] = vals
    return out


# ---- sums for the kernel tests ---------------------------------------------------------------------------------------------------------------
def theta_sums(nat1, nat2, plin, pdiag, psub):
    """(lin [B, M, d], diag [B, M, d, d], sub [B, M, d, d] with a zero last block, sums of absolute terms of each)."""
    d = plin.shape[-1]
    M = plin.shape[0]
    lin = plin + nat1[:, 1:, :d] + nat1[:, :-1, d:]
    alin = np.abs(plin) + np.abs(nat1[:, 1:, :d]) + np.abs(nat1[:, :-1, d:])
    diag = pdiag + nat2[:, 1:, :d, :d] + nat2[:, :-1, d:, d:]
    adiag = np.abs(pdiag) + np.abs(nat2[:, 1:, :d, :d]) + np.abs(nat2[:, :-1, d:, d:])
    sub, asub = np.zeros_like(diag), np.zeros_like(diag)
    sub[:, :M - 1] = psub[:M - 1] + 2.0 * nat2[:, 1:M, d:, :d]
    asub[:, :M - 1] = np.abs(psub[:M - 1]) + 2.0 * np.abs(nat2[:, 1:M, d:, :d])
    return lin, diag, sub, alin, adiag, asub


def pairs(mu, Sig, Sub, pm, P0):
    """Pair means [B, M + 1, 2d] and covariances [B, M + 1, 2d, 2d] from the chain blocks mu [B, M, d], Sig [B, M, d, d], Sub
    [B, M, d, d] (Sigma_{t+1,t} at t): the prior's (pm, P0) at both ends, zero cross block there."""
    B, M, d = mu.shape
    pmu, pair = np.zeros((B, M + 1, 2 * d)), np.zeros((B, M + 1, 2 * d, 2 * d))
    for m in range(M + 1):
        pmu[:, m, :d] = pm if m == 0 else mu[:, m - 1]
        pmu[:, m, d:] = pm if m == M else mu[:, m]
        pair[:, m, :d, :d] = P0 if m == 0 else Sig[:, m - 1]
        pair[:, m, d:, d:] = P0 if m == M else Sig[:, m]
        if 0 < m < M:
            pair[:, m, d:, :d] = Sub[:, m - 1]
            pair[:, m, :d, d:] = Sub[:, m - 1].transpose(0, 2, 1)
    return pmu, pair


def predict_sums(w, c, idx, pmu, pair):
    """(fmu, fvar [B, N], sums of absolute terms of each)."""
    rows = np.arange(w.shape[0])[:, None]
    pm, pc = pmu[rows, idx], pair[rows, idx]
    fmu = np.einsum("bnj,bnj->bn", w, pm)
    smu = np.einsum("bnj,bnj->bn", np.abs(w), np.abs(pm))
    fvar = c + np.einsum("bni,bnij,bnj->bn", w, pc, w)
    svar = np.abs(c) + np.einsum("bni,bnij,bnj->bn", np.abs(w), np.abs(pc), np.abs(w))
    return fmu, fvar, smu, svar


def site_sums(w, idx, g1, g2, nat1, nat2, lr):
    """(nat1, nat2, sums of absolute terms of each) after one update."""
    B, M1 = nat1.shape[:2]
    s1, a1, s2, a2 = np.zeros_like(nat1), np.zeros_like(nat1), np.zeros_like(nat2), np.zeros_like(nat2)
    rows = np.broadcast_to(np.arange(B)[:, None], idx.shape)
    np.add.at(s1, (rows, idx), g1[..., None] * w)
    np.add.at(a1, (rows, idx), np.abs(g1[..., None] * w))
    outer = w[..., :, None] * w[..., None, :]
    np.add.at(s2, (rows, idx), g2[..., None, None] * outer)
    np.add.at(a2, (rows, idx), np.abs(g2[..., None, None] * outer))
    return (1 - lr) * nat1 + lr * s1, (1 - lr) * nat2 + lr * s2, np.abs((1 - lr) * nat1) + lr * a1, np.abs((1 - lr) * nat2) + lr * a2
