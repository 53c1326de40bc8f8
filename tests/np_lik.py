"""
NumPy / SciPy restatement of the scalar non-Gaussian likelihoods (include/mfgm.h, mfgm_scalar_lik; gpflow.likelihoods.Bernoulli with the
probit link and jitter, gpflow.likelihoods.Poisson with the exp link).  Duck-typed like oracle/np_models.GaussianLik, so that it plugs
into the oracle CVI models unchanged: variational_expectations(mu, var, y) and grads_expectation(mu, var, y) -> (g1, g2).
"""
import numpy as np
from scipy import special

XI, WH = np.polynomial.hermite.hermgauss(20)
W = WH / np.sqrt(np.pi)


def nodes(mu, var):
    """X [..., 20] = mu + sqrt(2) sigma xi_k."""
    return np.asarray(mu)[..., None] + np.sqrt(2.0) * np.sqrt(np.asarray(var))[..., None] * XI


def phi_cdf(x):
    return 0.5 * special.erfc(-x / np.sqrt(2.0))


class Bernoulli:
    def __init__(self, jitter=1e-3):
        self.j = float(jitter)

    def p(self, f):
        return self.j + (1.0 - 2.0 * self.j) * phi_cdf(f)

    def terms(self, mu, var, y):
        """Per-node quantities of the rule: (X, W l(X), W l'(X)) [..., 20]."""
        X = nodes(mu, var)
        s = np.where(np.asarray(y)[..., None] == 1, 1.0, -1.0)
        p = self.p(s * X)
        dl = s * (1.0 - 2.0 * self.j) * np.exp(-0.5 * X * X) / np.sqrt(2.0 * np.pi) / p
        return X, W * np.log(p), W * dl

    def ve_and_grads(self, mu, var, y):
        """(VE, dVE/dmu, dVE/dv) and the scales of the two sums (sum of absolute terms) for relative comparisons."""
        _, l, dl = self.terms(mu, var, y)
        sc = np.sqrt(2.0) * np.sqrt(var)
        # log p is taken of p rounded to fp64: its error is ~u (|log p| + 1), which is what the VE scale sums (for p near 1, as at j = 0
        # and a large s X, |log p| alone is far below that rounding)
        return (l.sum(-1), dl.sum(-1), (dl * XI).sum(-1) / sc,
                dict(ve=(np.abs(l) + W).sum(-1), dmu=np.abs(dl).sum(-1), dv=np.abs(dl * XI).sum(-1) / sc))

    def variational_expectations(self, mu, var, y):
        return self.ve_and_grads(mu, var, y)[0]

    def grads_expectation(self, mu, var, y):
        _, dmu, dv, _ = self.ve_and_grads(mu, var, y)
        return dmu - 2.0 * dv * mu, dv

    def predict_mean_and_var(self, mu, var):
        p = self.p(mu / np.sqrt(1.0 + var))
        return p, p - p * p

    def predict_log_density(self, mu, var, y):
        x = mu / np.sqrt(1.0 + var)
        return np.log(self.p(np.where(y == 1, x, -x))).sum(-1)


class Poisson:
    def __init__(self, binsize=1.0):
        self.b = float(binsize)

    def log_prob(self, F, Y):
        return Y * (np.log(self.b) + F) - self.b * np.exp(F) - special.gammaln(Y + 1.0)

    def ve_and_grads(self, mu, var, y):
        m = self.b * np.exp(mu + 0.5 * var)
        ve = y * np.log(self.b) + y * mu - m - special.gammaln(y + 1.0)
        return (ve, y - m, -0.5 * m,
                dict(ve=np.abs(y * np.log(self.b)) + np.abs(y * mu) + m + special.gammaln(y + 1.0), dmu=np.abs(y) + m, dv=0.5 * m))

    def variational_expectations(self, mu, var, y):
        return self.ve_and_grads(mu, var, y)[0]

    def grads_expectation(self, mu, var, y):
        _, dmu, dv, _ = self.ve_and_grads(mu, var, y)
        return dmu - 2.0 * dv * mu, dv

    def predict_mean_and_var(self, mu, var):
        m = self.b * np.exp(mu + 0.5 * var)
        return m, m + np.expm1(var) * m * m

    def predict_log_density(self, mu, var, y):
        X = nodes(mu, var)
        return special.logsumexp(np.log(W) + self.log_prob(X, np.asarray(y)[..., None]), axis=-1).sum(-1)
