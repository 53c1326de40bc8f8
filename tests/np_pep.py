"""
NumPy restatement of Power Expectation Propagation on the sites-on-f GP model (include/mfgm.h, mfgm_pep_sites; vidp_amd.pep).  It
restates the reference's update (markovflow/models/pep.py:179-215, gradient_correction :250-261) literally, with two differences: the
tilted normaliser is the exact integral log int p(y|f)^alpha N(f; mc, vc) df, and the energy's per-point terms are taken at the cavity.
The reference's own formulas are kept next to them (`*_reference`) for the tests that show where they differ.

Likelihood kinds: "gaussian" (param = variance), "bernoulli" (probit, param = jitter), "poisson" (exp link, param = bin size).
"""
import numpy as np
from scipy import special

from oracle import np_kalman

XI20, WH20 = np.polynomial.hermite.hermgauss(20)
LOG2PI = np.log(2.0 * np.pi)


def phi_cdf(x):
    return 0.5 * special.erfc(-x / np.sqrt(2.0))


def loglik(kind, X, y, param):
    """(l, l', l'') of log p(y | f) at f = X (broadcasting)."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if kind == "gaussian":
        r = y - X
        return -0.5 * (LOG2PI + np.log(param)) - 0.5 * r * r / param, r / param, -np.ones_like(X + y) / param
    if kind == "bernoulli":
        s = np.where(y == 1, 1.0, -1.0)
        c = 1.0 - 2.0 * param
        p = param + c * phi_cdf(s * X)
        dl = s * c * np.exp(-0.5 * X * X) / np.sqrt(2.0 * np.pi) / p
        return np.log(p), dl, -X * dl - dl * dl
    m = param * np.exp(X)
    return y * (np.log(param) + X) - m - special.gammaln(y + 1.0), y - m, -m


def tilted_rule(kind, mc, vc, y, param, alpha, n_gh=20):
    """log Z, d1, d2 by the n_gh-point rule in log space and its derivatives (gpflow's quadrature.logspace under a double tape), and
    the scales (sums of absolute terms) of d1 and d2 for relative comparisons."""
    xi, w = np.polynomial.hermite.hermgauss(n_gh)
    X = np.asarray(mc)[..., None] + np.sqrt(2.0 * np.asarray(vc))[..., None] * xi
    l, dl, d2l = loglik(kind, X, np.asarray(y)[..., None], param)
    a = np.log(w / np.sqrt(np.pi)) + alpha * l
    lz = special.logsumexp(a, axis=-1)
    pi = np.exp(a - lz[..., None])
    g1, g2 = alpha * dl, alpha * d2l + (alpha * dl) ** 2
    d1 = (pi * g1).sum(-1)
    d2 = (pi * g2).sum(-1) - d1 * d1
    return lz, d1, d2, dict(d1=(pi * np.abs(g1)).sum(-1), d2=(pi * np.abs(g2)).sum(-1) + d1 * d1)


def tilted(kind, mc, vc, y, param, alpha, n_gh=20):
    """log Z, d1, d2 as the contract defines them (closed forms for Gaussian and for Bernoulli at alpha = 1) and their scales."""
    mc, vc, y = (np.asarray(v, dtype=np.float64) for v in (mc, vc, y))
    if kind == "gaussian":
        S = param / alpha + vc
        r = y - mc
        lz = 0.5 * (1.0 - alpha) * (LOG2PI + np.log(param)) - 0.5 * np.log(alpha) - 0.5 * (LOG2PI + np.log(S)) - 0.5 * r * r / S
        return lz, r / S, -1.0 / S, dict(d1=np.abs(r) / S, d2=1.0 / S)
    if kind == "bernoulli" and alpha == 1.0:
        s = np.where(y == 1, 1.0, -1.0)
        c = 1.0 - 2.0 * param
        q = 1.0 / np.sqrt(1.0 + vc)
        z = s * mc * q
        p = param + c * phi_cdf(z)
        g = c * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) / p
        return np.log(p), s * q * g, (-z * g - g * g) * q * q, dict(d1=q * g, d2=(np.abs(z * g) + g * g) * q * q)
    return tilted_rule(kind, mc, vc, y, param, alpha, n_gh)


def tilted_brute(kind, mc, vc, y, param, alpha, n=40001, width=14.0):
    """log Z, d1, d2 of one point by the trapezoid rule on a fine grid: d1 = E~[f - mc] / vc, d2 = Var~[f] / vc^2 - 1 / vc under the
    tilted density p(y|f)^alpha N(f; mc, vc) / Z."""
    sd = np.sqrt(vc)
    f = mc + sd * np.linspace(-width, width, n)
    l = alpha * loglik(kind, f, y, param)[0] - 0.5 * (f - mc) ** 2 / vc - 0.5 * np.log(2.0 * np.pi * vc)
    m = l.max()
    g = np.exp(l - m)
    trap = lambda u: (f[1] - f[0]) * (u.sum() - 0.5 * (u[0] + u[-1]))
    Z = trap(g)
    E = trap(g * (f - mc)) / Z
    V = trap(g * (f - mc) ** 2) / Z - E * E
    return m + np.log(Z), E / vc, V / vc ** 2 - 1.0 / vc


def tilted_reference(kind, mc, vc, y, param, alpha):
    """The reference's log_expected_density and gradients: PEPGaussian's alpha log N(y; mc, s^2 + vc), (alpha (y - mc) / var,
    -alpha / var); PEPScalarLikelihood's base.predict_log_density (alpha ignored: closed form for Bernoulli, the 20-point rule of
    log p for Poisson)."""
    if kind == "gaussian":
        var = param + vc
        return alpha * (-0.5 * (LOG2PI + np.log(var)) - 0.5 * (y - mc) ** 2 / var), alpha * (y - mc) / var, -alpha / var
    return tilted(kind, mc, vc, y, param, 1.0)[:3]


def cavity_f(mu, v, nat1, nat2, alpha):
    """(mc, vc, lc): the cavity of q(f) / t(f)^alpha in f-space (Sherman-Morrison form of the state-space cavity)."""
    lc = 1.0 / v + 2.0 * alpha * nat2
    vc = 1.0 / lc
    return vc * (mu / v - alpha * nat1), vc, lc


def cavity_state(means, covs, H, nat1, nat2, alpha):
    """The reference's state-space cavity (pep.py:115-147): per-state posterior naturals minus alpha times the back-projected site,
    back to moments, projected by H [..., 1, d]; nat1, nat2 [...]."""
    P = np.linalg.inv(covs)
    n2 = -0.5 * P
    n1 = (P @ means[..., None])[..., 0]
    h = H[..., 0, :]
    cav_n2 = n2 - alpha * nat2[..., None, None] * h[..., :, None] * h[..., None, :]
    cav_n1 = n1 - alpha * nat1[..., None] * h
    C = np.linalg.inv(-2.0 * cav_n2)
    m = (C @ cav_n1[..., None])[..., 0]
    return (h * m).sum(-1), np.einsum("...i,...ij,...j->...", h, C, h)


def log_norm_1d(m, v):
    return 0.5 * (np.log(v) + m * m / v)


def gradient_correction(inputs, grads):
    L2 = 0.5 / (inputs[1] + 1.0 / grads[1])
    return 2.0 * L2 * (grads[0] / grads[1] - inputs[0]), L2


def site_update(kind, mu, v, y, nat1, nat2, lnorm, param, alpha, lr):
    """One PEP update at every given point: (new nat1, new nat2, new lnorm, e, ok); a point with an improper cavity or non-finite
    moments keeps its site (ok False, e NaN)."""
    with np.errstate(all="ignore"):
        mc, vc, lc = cavity_f(mu, v, nat1, nat2, alpha)
        lz, d1, d2, _ = tilted(kind, mc, vc, y, param, alpha)
        L1, L2 = gradient_correction([mc, vc], [d1, d2])
        e = lz + log_norm_1d(mc, vc) - log_norm_1d(mu, v)
    ok = (v > 0) & (lc > 0) & np.isfinite(L1) & np.isfinite(L2)
    new1 = (1 - lr) * nat1 + lr * ((1 - alpha) * nat1 + L1)
    new2 = (1 - lr) * nat2 + lr * ((1 - alpha) * nat2 + L2)
    new3 = (1 - lr) * lnorm + lr * ((1 - alpha) * lnorm + e)
    return (np.where(ok, new1, nat1), np.where(ok, new2, nat2), np.where(ok, new3, lnorm), np.where(ok, e, np.nan), ok)


def normalizer(Lam, mu):
    """1/2 (dim log 2 pi - log det Lambda + mu^T Lambda mu) (state_space_model.py:595-609 of the reference)."""
    return 0.5 * (len(mu) * LOG2PI - np.linalg.slogdet(Lam)[1] + mu @ Lam @ mu)


def dense_precision(ssm):
    """The prior precision of an oracle StateSpaceModel (one chain) as a dense [T d, T d] matrix."""
    pd, ps = ssm.precision()
    T, d = pd.shape[0], pd.shape[-1]
    P = np.zeros((T * d, T * d))
    for t in range(T):
        P[t * d:(t + 1) * d, t * d:(t + 1) * d] = pd[t]
    for t in range(T - 1):
        P[(t + 1) * d:(t + 2) * d, t * d:(t + 1) * d] = ps[t]
        P[t * d:(t + 1) * d, (t + 1) * d:(t + 2) * d] = ps[t].T
    return P


class PowerExpectationPropagation:
    """pep.py:28-247 on one chain, dense: the posterior precision is the prior's plus the back-projected sites, inverted outright."""

    def __init__(self, time_points, observations, kernel, kind, param, learning_rate=1.0, alpha=1.0):
        self.t = np.asarray(time_points, dtype=np.float64)
        self.y = np.asarray(observations, dtype=np.float64).reshape(-1)
        self.kernel, self.kind, self.param, self.lr, self.alpha = kernel, kind, float(param), learning_rate, alpha
        n = len(self.t)
        self.nat1, self.nat2, self.log_norm = np.zeros(n), -1e-10 * np.ones(n), np.zeros(n)
        self.ssm = kernel.state_space_model(self.t)
        self.Pp = dense_precision(self.ssm)
        self.d = kernel.state_dim

    def posterior(self):
        """(Lambda_q, mu_q, Sigma_q) of the states."""
        n, d = len(self.t), self.d
        P = self.Pp.copy()
        b = np.zeros(n * d)
        P[np.arange(n) * d, np.arange(n) * d] += -2.0 * self.nat2
        b[np.arange(n) * d] = self.nat1
        S = np.linalg.inv(P)
        return P, S @ b, S

    def predict_f(self):
        _, mu, S = self.posterior()
        i = np.arange(len(self.t)) * self.d
        return mu[i], S[i, i]

    def update_sites(self, site_indices=None):
        mu, v = self.predict_f()
        n1, n2, ln, _, _ = site_update(self.kind, mu, v, self.y, self.nat1, self.nat2, self.log_norm, self.param, self.alpha, self.lr)
        sel = np.ones(len(self.t), bool) if site_indices is None else np.isin(np.arange(len(self.t)), np.asarray(site_indices).ravel())
        self.nat1, self.nat2, self.log_norm = np.where(sel, n1, self.nat1), np.where(sel, n2, self.nat2), np.where(sel, ln, self.log_norm)

    def elbo(self):
        sites = np_kalman.GaussianSitesNat(self.nat1[:, None], self.nat2[:, None, None])
        return np_kalman.KalmanFilterWithSites(self.ssm, self.kernel.emission_matrix(self.t), sites).log_likelihood()

    def log_norm_terms(self):
        mu, v = self.predict_f()
        mc, vc, _ = cavity_f(mu, v, self.nat1, self.nat2, self.alpha)
        lz = tilted(self.kind, mc, vc, self.y, self.param, self.alpha)[0]
        return lz + log_norm_1d(mc, vc) - log_norm_1d(mu, v)

    def log_norm_terms_reference(self):
        """The reference's compute_log_norm: the tilted normaliser (its own formula) at the posterior marginal."""
        mu, v = self.predict_f()
        mc, vc, _ = cavity_f(mu, v, self.nat1, self.nat2, self.alpha)
        return tilted_reference(self.kind, mu, v, self.y, self.param, self.alpha)[0] + log_norm_1d(mc, vc) - log_norm_1d(mu, v)

    def energy(self, reference=False):
        P, mu, _ = self.posterior()
        e = self.log_norm_terms_reference() if reference else self.log_norm_terms()
        return normalizer(P, mu) - normalizer(self.Pp, np.zeros(len(mu))) + e.sum() / self.alpha
