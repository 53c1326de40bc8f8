"""
NumPy restatement of the linear-readout likelihood of the diffusion models (include/mfgm.h, mfgm_readout; vidp_amd.likelihoods.
LinearReadout) on top of tests/np_lik.py, and the oracle models CVISitesSSM / CVISitesSDE with an observation dimension of their own.

    p(y_i | x_i) = prod_j p_j(y_ij | h_j^T x_i + c_j);  per observation with marginal N(mu, Sigma):
    m_j = h_j^T mu + c_j,  v_j = h_j^T Sigma h_j,  (ve_j, dm_j, dv_j) of the scalar factor at (m_j, v_j, y_ij), 0 where y_ij is NaN,
    VE = sum_j ve_j,   g2 = sum_j dv_j h_j h_j^T,   g1 = sum_j h_j (dm_j - 2 dv_j h_j^T mu).

Next to every quantity comes its scale, the sum of the absolute values of the terms it is summed from (np_lik's scales of the scalar
quantities carried through the sums above): comparisons are made against 1e-12 of that, as in tests/test_host_lik.py.
"""
import numpy as np

from oracle import np_models
from tests import np_lik


class Gaussian:
    """Scalar Gaussian factor with variance s^2, in the interface of np_lik.Bernoulli / Poisson."""

    def __init__(self, variance):
        self.s2 = float(variance)

    def ve_and_grads(self, mu, var, y):
        r = y - mu
        ve = -0.5 * np.log(2 * np.pi * self.s2) - 0.5 * (r * r + var) / self.s2
        dv = -0.5 / self.s2 * np.ones_like(var)
        return (ve, r / self.s2, dv,
                dict(ve=0.5 * abs(np.log(2 * np.pi * self.s2)) + 0.5 * (r * r + np.abs(var)) / self.s2,
                     dmu=(np.abs(y) + np.abs(mu)) / self.s2, dv=np.abs(dv)))

    def predict_mean_and_var(self, mu, var):
        return mu, var + self.s2

    def predict_log_density(self, mu, var, y):
        s = var + self.s2
        return (-0.5 * np.log(2 * np.pi * s) - 0.5 * (y - mu) ** 2 / s).sum(-1)


class LinearReadout:
    """Duck-typed like oracle/np_models.MultivariateGaussianLik: variational_expectations(mu, cov, y), grads_expectation(mu, cov, y)."""

    def __init__(self, H, liks, offset=None):
        self.H = np.asarray(H, dtype=np.float64)
        self.o, self.d = self.H.shape
        self.c = np.zeros(self.o) if offset is None else np.asarray(offset, dtype=np.float64)
        self.liks = list(liks) if isinstance(liks, (list, tuple)) else [liks] * self.o

    def project(self, mu, cov):
        return mu @ self.H.T + self.c, np.einsum("od,...de,oe->...o", self.H, cov, self.H)

    def outputs(self, mu, cov, y):
        """Per output [n, o]: (ve, dm, dv, h^T mu) and their scales (dict ve / dmu / dv), zero where y is NaN."""
        y = np.asarray(y, dtype=np.float64)
        m, v = self.project(mu, cov)
        seen = ~np.isnan(y)
        ys = np.where(seen, y, 0.0)
        cols = [b.ve_and_grads(m[..., j], v[..., j], ys[..., j]) for j, b in enumerate(self.liks)]
        stack = lambda k: np.where(seen, np.stack([np.broadcast_to(c[k], m[..., 0].shape) for c in cols], -1), 0.0)
        sc = {k: np.where(seen, np.stack([np.broadcast_to(c[3][k], m[..., 0].shape) for c in cols], -1), 0.0) for k in ("ve", "dmu", "dv")}
        return stack(0), stack(1), stack(2), m - self.c, sc

    def all_with_scales(self, mu, cov, y):
        """(VE [n], g1 [n, d], g2 [n, d, d]) and their scales (the same shapes)."""
        ve, dm, dv, hm, sc = self.outputs(mu, cov, y)
        H, aH = self.H, np.abs(self.H)
        g1 = (dm - 2.0 * dv * hm) @ H
        g2 = np.einsum("...o,or,oc->...rc", dv, H, H)
        s1 = (sc["dmu"] + 2.0 * sc["dv"] * np.abs(hm)) @ aH
        s2 = np.einsum("...o,or,oc->...rc", sc["dv"], aH, aH)
        return (ve.sum(-1), g1, g2), (sc["ve"].sum(-1), s1, s2)

    def variational_expectations(self, mu, cov, y):
        return self.outputs(mu, cov, y)[0].sum(-1)

    def grads_expectation(self, mu, cov, y):
        _, g1, g2 = self.all_with_scales(mu, cov, y)[0]
        return g1, g2

    def predict_mean_and_var(self, mu, cov):
        m, v = self.project(mu, cov)
        out = [b.predict_mean_and_var(m[..., j], v[..., j]) for j, b in enumerate(self.liks)]
        return np.stack([a for a, _ in out], -1), np.stack([e for _, e in out], -1)

    def predict_log_density(self, mu, cov, y):
        y = np.asarray(y, dtype=np.float64)
        m, v = self.project(mu, cov)
        seen = ~np.isnan(y)
        ys = np.where(seen, y, 0.0)
        lp = np.stack([b.predict_log_density(m[..., j:j + 1], v[..., j:j + 1], ys[..., j:j + 1]) for j, b in enumerate(self.liks)], -1)
        return np.where(seen, lp, 0.0).sum(-1)


def nlpd_rmse(lik, mu, cov, y):
    """trainers._Metrics under a readout: minus the mean log predictive density of the points, and the root mean squared error of the
    predicted output means over the observed entries."""
    y = np.asarray(y, dtype=np.float64)
    seen = ~np.isnan(y)
    err = np.where(seen, lik.predict_mean_and_var(mu, cov)[0] - np.where(seen, y, 0.0), 0.0)
    return -np.mean(lik.predict_log_density(mu, cov, y)), np.sqrt((err ** 2).sum() / seen.sum())


class CVISitesSSM(np_models.CVISitesSSM):
    """oracle CVISitesSSM with y [n, o] and a likelihood that names the state dimension (the oracle class reads d from y: it is built on
    a [n, d] placeholder and handed the observations afterwards)."""

    def __init__(self, prior_ssm, time_grid, obs_index, observations, likelihood):
        y = np.asarray(observations, dtype=np.float64)
        super().__init__(prior_ssm, time_grid, obs_index, np.zeros((y.shape[0], likelihood.d)), likelihood)
        self.y = y


class CVISitesSDE(np_models.CVISitesSDE):
    def __init__(self, prior_sde, time_grid, obs_index, observations, likelihood, init_mu, init_cov, **kw):
        y = np.asarray(observations, dtype=np.float64)
        super().__init__(prior_sde, time_grid, obs_index, np.zeros((y.shape[0], likelihood.d)), likelihood, init_mu, init_cov, **kw)
        self.y = y


def random_readout(rng, d, o, kinds="gpb", offset=True):
    """(torch-side factory arguments, NumPy readout): H ~ N(0, 1) / sqrt(d), kinds cycled over the outputs (g Gaussian, p Poisson,
    b Bernoulli)."""
    H = rng.normal(size=(o, d)) / np.sqrt(d)
    c = rng.uniform(-0.5, 0.5, size=o) if offset else None
    spec = []
    for j in range(o):
        k = kinds[j % len(kinds)]
        spec.append((k, {"g": 0.3 + 0.2 * j, "p": 0.7 + 0.1 * j, "b": 1e-3}[k]))
    liks = [{"g": Gaussian, "p": np_lik.Poisson, "b": np_lik.Bernoulli}[k](p) for k, p in spec]
    return H, c, spec, LinearReadout(H, liks, c)


def torch_readout(L, H, c, spec):
    """vidp_amd.likelihoods.LinearReadout of a `random_readout` description."""
    liks = [{"g": L.Gaussian, "p": L.Poisson, "b": L.Bernoulli}[k](p) for k, p in spec]
    return L.LinearReadout(H, liks, c)


def random_observations(rng, ref, mu, nan_frac=0.1):
    """y [n, o] matching the kinds (real, counts, labels), a fraction of the entries NaN."""
    n = mu.shape[0]
    y = np.empty((n, ref.o))
    for j, b in enumerate(ref.liks):
        if isinstance(b, Gaussian):
            y[:, j] = rng.normal(size=n)
        elif isinstance(b, np_lik.Poisson):
            y[:, j] = rng.poisson(2.0, size=n)
        else:
            y[:, j] = rng.integers(0, 2, size=n)
    y[rng.uniform(size=y.shape) < nan_frac] = np.nan
    return y


def random_marginals(rng, n, d):
    """mu [n, d] in [-1.5, 1.5], Sigma = A A^T / d + 0.1 I: v_j >= 0.1 |h_j|^2, so the projections are well conditioned and their
    rounding (a few ulp of sum |h| |Sigma| |h|) stays far inside the 1e-12 bounds of the quantities computed from them."""
    mu = rng.uniform(-1.5, 1.5, size=(n, d))
    A = rng.normal(size=(n, d, d))
    return mu, A @ np.swapaxes(A, -1, -2) / d + 0.1 * np.eye(d)
