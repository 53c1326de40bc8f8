"""
Host-side mirror of the Gaussian likelihoods on the path (markovflow/likelihoods/multivariate_gaussian.py:80-115;
gpflow.likelihoods.Gaussian for the scalar CVI-GP case): variational expectations and their gradients in
closed form (the reference differentiates them with a GradientTape, variational_cvi_sde.py:204-220).
Observation counts are tiny next to the time grid (n_obs << T), so these run as small batched torch ops on
the gathered observation nodes.

The scalar non-Gaussian likelihoods of the CVI models (Bernoulli, Poisson; gpflow.likelihoods) follow at the end: 20-point
Gauss-Hermite variational expectations and their site gradients, natively in one launch (mfgm_scalar_lik).

LinearReadout, last, lets the diffusion models see their state through f = H x + c with one of these scalar likelihoods per output
(DESIGN.md section 19).

MultiStageLikelihood and HeteroskedasticGaussian, at the end, couple several latent GPs at one observation: the likelihoods of
MultiLatentSparseCVI.
"""
import math

import torch

from . import _lib, linalg
from .packed import _ptr, _stream
from .stamps import Stamp


class MultivariateGaussian:
    """p(y | f) = N(y; f, L L^T) (multivariate_gaussian.py:29-160)."""

    # d VE / d(eta) = (S^{-1} y, -1/2 S^{-1}) does not depend on q, and its second part is the same block for every observation: the
    # CVI-DP model then keeps the data sites out of the per-node arrays (variational_cvi_sde.CVISitesSDE, cq state)
    uniform_site_gradient = True

    def __init__(self, chol_covariance):
        self.chol_covariance = chol_covariance

    @property
    def chol_covariance(self):
        return self._chol

    @chol_covariance.setter
    def chol_covariance(self, chol_covariance):
        """Everything derived from the factor is rebuilt when it is replaced (no stale inverse / constant / gradient cache)."""
        self._chol = chol_covariance
        self.obs_dim = chol_covariance.shape[-1]
        # one d x d inverse, reused by every call (no per-observation triangular solves)
        self.inv_covariance = linalg.spd_inverse(chol=chol_covariance)
        self.log_det_chol = torch.log(torch.diagonal(chol_covariance)).sum()
        # additive constant of the variational expectations, as a host scalar (one synchronisation, here)
        self.ve_constant = -float(self.log_det_chol) - 0.5 * self.obs_dim * math.log(2.0 * math.pi)
        self._g_cache = None

    def predict_mean_and_var(self, f_means, f_covariances):
        """Marginals of y (multivariate_gaussian.py:117-136): (f_means, f_covariances + L L^T), or with marginal variances
        ([..., n, d]) the diagonal of L L^T added."""
        cov = self._chol @ self._chol.T
        if f_covariances.dim() == f_means.dim():
            return f_means, f_covariances + torch.diagonal(cov)
        return f_means, f_covariances + cov

    def variational_expectations(self, f_means, f_covariances, observations):
        """-1/2 tr(S^{-1} S_i) + log N(y_i; mu_i, S) (multivariate_gaussian.py:80-115); shape [..., n]."""
        Sinv = self.inv_covariance
        diff = observations - f_means
        # element-wise d x d contraction (a [n, d] x [d, d] GEMM call costs ~0.2 ms of launch-bound rocBLAS time at n ~ 1e5)
        quad = (diff[..., :, None] * Sinv * diff[..., None, :]).sum(dim=(-1, -2))
        logp = -0.5 * quad - self.log_det_chol - 0.5 * self.obs_dim * math.log(2 * math.pi)
        return -0.5 * (Sinv * f_covariances).sum(dim=(-1, -2)) + logp

    def ve_gradients_expectation(self, f_means, f_covariances, observations):
        """
        Gradient of sum_i VE_i with respect to the expectation parameters (mu, S + mu mu^T):
        d/dmu = S^{-1}(y - mu), d/dS = -1/2 S^{-1}, then gradient_transformation_mean_var_to_expectation
        (variational_cvi.py:448-462): g1 = d/dmu - 2 (d/dS) mu = S^{-1} y,  g2 = -1/2 S^{-1}.
        """
        # both gradients depend on the observations only: computed once per observation TENSOR OBJECT and version (a raw address
        # is no key: the caching allocator hands freed blocks back at the same address with the same shape)
        c, Sinv = self._g_cache, self.inv_covariance
        if c is None or not c[0].matches(observations, tuple(f_covariances.shape), Sinv):
            g1 = (Sinv * observations[..., None, :]).sum(-1)           # S^{-1} y (S symmetric)
            g2 = (-0.5 * Sinv).expand(f_covariances.shape).contiguous()
            c = self._g_cache = (Stamp(observations, tuple(f_covariances.shape), Sinv), g1, g2)
        return c[1], c[2]


class Gaussian:
    """Scalar Gaussian likelihood with variance `variance` (gpflow.likelihoods.Gaussian), obs_dim 1."""

    def __init__(self, variance):
        self.variance = float(variance)

    def predict_mean_and_var(self, f_means, f_vars):
        """(f_means, f_vars + variance) (gpflow.likelihoods.Gaussian)."""
        return f_means, f_vars + self.variance

    def variational_expectations(self, f_means, f_vars, observations):
        v = self.variance
        return -0.5 * math.log(2 * math.pi) - 0.5 * math.log(v) - 0.5 * ((observations - f_means) ** 2 + f_vars) / v

    def variational_expectations_terms(self, f_means, f_vars, observations):
        """(c, w, [t1, t2]) with  sum of variational_expectations = c + w (t1 + t2): the two reductions |y - m|^2 and sum var as device
        scalars, for callers that assemble their bound in one launch (mfgm_combine_terms)."""
        v = self.variance
        r = (observations - f_means).reshape(-1)
        return -0.5 * r.numel() * (math.log(2 * math.pi) + math.log(v)), -0.5 / v, [torch.dot(r, r).reshape(1), f_vars.sum().reshape(1)]

    def variational_expectations_sum(self, f_means, f_vars, observations):
        """sum of variational_expectations over all points, from two reductions instead of seven element-wise passes and one."""
        c, w, (t1, t2) = self.variational_expectations_terms(f_means, f_vars, observations)
        return c + w * (t1 + t2)[0]

    def ve_gradients_expectation(self, f_means, f_vars, observations):
        # (y / v, -1/2 / v) depend on the observations only: computed once per observation tensor object and version
        v = self.variance
        c = getattr(self, "_g_cache", None)
        if c is None or not c[0].matches(observations, tuple(f_vars.shape), v):
            c = self._g_cache = (Stamp(observations, tuple(f_vars.shape), v), observations / v, torch.full_like(f_vars, -0.5 / v))
        return c[1], c[2]


# ---- scalar non-Gaussian likelihoods (gpflow.likelihoods.Bernoulli / Poisson, the ones the reference's CVI walkthroughs fit) ----------
class ScalarQuadratureLikelihood:
    """A scalar likelihood p(y | f) given by its log density `log_prob(F, Y)` (a torch function, broadcasting), with the variational
    expectations taken by the n_gh-point Gauss-Hermite rule of gpflow's NDiagGHQuadrature (include/mfgm.h, mfgm_scalar_lik):
        X_k = mu + sqrt(2) sigma xi_k,   VE = sum_k W_k log_prob(X_k, y),   W_k = w_k / sqrt(pi)
    and the site gradients by autograd through that rule -- what the reference's GradientTape over
    likelihood.variational_expectations gives (variational_cvi.py:332-349).  The generic route: torch only.  Shapes as Gaussian:
    f_means, f_vars, observations [..., n, 1]; variational_expectations [..., n]; (g1, g2) [..., n, 1].  v <= 0 is not clamped.

    Subclasses with a `kind` (Bernoulli, Poisson) run the same quantities in one HIP launch (mfgm_scalar_lik) when the tensors are on
    the device, contiguous fp64, and nothing asks for a gradient; otherwise they take this torch route, which stays differentiable
    (classic_elbo_tape, ssm_natgrad).  The gradients depend on q: nothing is cached across calls."""

    kind = None          # mfgm_scalar_lik kind of the native route; None: torch only

    def __init__(self, log_prob, n_gh=20):
        import numpy as np
        self.log_prob = log_prob
        self.n_gh = int(n_gh)
        xi, w = np.polynomial.hermite.hermgauss(self.n_gh)
        self._xi, self._w = xi, w / math.sqrt(math.pi)
        self._rule_cache = {}

    @property
    def param(self):
        """The scalar parameter handed to mfgm_scalar_lik (jitter / bin size)."""
        raise NotImplementedError

    def _rule(self, like):
        """(xi, W) as tensors on `like`'s device: constants of the rule (not of q), made once per device."""
        key = str(like.device)
        r = self._rule_cache.get(key)
        if r is None:
            r = self._rule_cache[key] = (torch.tensor(self._xi, dtype=torch.float64, device=like.device),
                                         torch.tensor(self._w, dtype=torch.float64, device=like.device))
        return r

    def _nodes(self, f_means, f_vars):
        xi, w = self._rule(f_means)
        return f_means[..., None] + math.sqrt(2.0) * torch.sqrt(f_vars)[..., None] * xi, w

    def _ve_torch(self, f_means, f_vars, observations):
        """[..., n, 1]: sum_k W_k log_prob(X_k, y) (differentiable)."""
        X, w = self._nodes(f_means, f_vars)
        return (self.log_prob(X, observations[..., None]) * w).sum(-1)

    # ---- native route ----------------------------------------------------------------------------------------------------------------
    def _native(self, f_means, f_vars, observations):
        if self.kind is None or not f_means.is_cuda:
            return False
        ts = (f_means, f_vars, observations)
        if any(t.requires_grad for t in ts) and torch.is_grad_enabled():
            return False
        return all(t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.shape == f_means.shape for t in ts)

    def _launch(self, f_means, f_vars, observations, ve=False, grads=False):
        n = f_means.numel()
        mk = lambda: torch.empty(f_means.shape, dtype=torch.float64, device=f_means.device)
        out_ve = mk() if ve else None
        g1, g2 = (mk(), mk()) if grads else (None, None)
        _lib.check(_lib.load().mfgm_scalar_lik(self.kind, n, _ptr(f_means), _ptr(f_vars), _ptr(observations), float(self.param),
                                               _ptr(out_ve), _ptr(g1), _ptr(g2), _stream()), "mfgm_scalar_lik")
        return out_ve, g1, g2

    # ---- interface of the CVI models -----------------------------------------------------------------------------------------------
    def variational_expectations(self, f_means, f_vars, observations):
        """E_q log p(y_i | f_i), [..., n]."""
        if self._native(f_means, f_vars, observations):
            return self._launch(f_means, f_vars, observations, ve=True)[0].sum(-1)
        return self._ve_torch(f_means, f_vars, observations).sum(-1)

    def variational_expectations_sum(self, f_means, f_vars, observations):
        """Sum of variational_expectations over every point, a device scalar (no host synchronisation)."""
        return self.variational_expectations(f_means, f_vars, observations).sum()

    def ve_gradients_expectation(self, f_means, f_vars, observations):
        """(g1, g2) = (dVE/dmu - 2 (dVE/dv) mu, dVE/dv), [..., n, 1] each: the gradient of sum_i VE_i with respect to the expectation
        parameters (mu, v + mu^2) (gradient_transformation_mean_var_to_expectation, variational_cvi.py:448-462)."""
        if self._native(f_means, f_vars, observations):
            _, g1, g2 = self._launch(f_means, f_vars, observations, grads=True)
            return g1, g2
        with torch.enable_grad():
            mu = f_means.detach().requires_grad_(True)
            v = f_vars.detach().requires_grad_(True)
            dmu, dv = torch.autograd.grad(self._ve_torch(mu, v, observations.detach()).sum(), [mu, v])
        return dmu - 2.0 * dv * f_means.detach(), dv

    def predict_log_density(self, f_means, f_vars, observations):
        """log int p(y | f) q(f) df by the rule in log space (gpflow's quadrature.logspace): logsumexp_k(log W_k + log_prob(X_k, y)),
        [..., n]."""
        X, w = self._nodes(f_means, f_vars)
        return torch.logsumexp(self.log_prob(X, observations[..., None]) + torch.log(w), dim=-1).sum(-1)

    def predict_mean_and_var(self, f_means, f_vars):
        raise NotImplementedError("a likelihood given by its log density alone has no closed-form predictive moments")


def _probit(x):
    """Phi(x) = erfc(-x / sqrt 2) / 2 (accurate in the lower tail, where 1/2 (1 + erf) is not)."""
    return 0.5 * torch.erfc(-x * (1.0 / math.sqrt(2.0)))


class Bernoulli(ScalarQuadratureLikelihood):
    """gpflow.likelihoods.Bernoulli with its default probit link and jitter j = 1e-3:  p_j(f) = j + (1 - 2j) Phi(f);  log p(y | f) =
    log p_j(f) for y == 1 and log(1 - p_j(f)) for any other y (gpflow's where(y == 1, p, 1 - p)), with 1 - p_j(f) computed as
    j + (1 - 2j) Phi(-f).  Variational expectations by the 20-point rule; natively on the device (mfgm_scalar_lik kind 1)."""

    kind = 1

    def __init__(self, jitter=1e-3):
        self.jitter = float(jitter)
        super().__init__(self._log_prob, n_gh=20)

    @property
    def param(self):
        return self.jitter

    def _p(self, f):
        return self.jitter + (1.0 - 2.0 * self.jitter) * _probit(f)

    def _log_prob(self, F, Y):
        return torch.log(self._p(torch.where(Y == 1, F, -F)))

    def predict_mean_and_var(self, f_means, f_vars):
        """p = p_j(mu / sqrt(1 + v)) and p - p^2 (closed form, gpflow.likelihoods.Bernoulli)."""
        p = self._p(f_means / torch.sqrt(1.0 + f_vars))
        return p, p - p * p

    def predict_log_density(self, f_means, f_vars, observations):
        """log Bernoulli(y; p), p = p_j(mu / sqrt(1 + v)) (closed form), 1 - p in the Phi(-x) form; [..., n]."""
        x = f_means / torch.sqrt(1.0 + f_vars)
        return torch.log(self._p(torch.where(observations == 1, x, -x))).sum(-1)


class Poisson(ScalarQuadratureLikelihood):
    """gpflow.likelihoods.Poisson with the exp link and bin size b:  log p(y | f) = y log(b e^f) - b e^f - lgamma(y + 1).  Variational
    expectations in closed form (as gpflow): VE = y log b + y mu - b e^{mu + v/2} - lgamma(y + 1); natively on the device
    (mfgm_scalar_lik kind 2)."""

    kind = 2

    def __init__(self, binsize=1.0):
        self.binsize = float(binsize)
        super().__init__(self._log_prob, n_gh=20)

    @property
    def param(self):
        return self.binsize

    def _log_prob(self, F, Y):
        return Y * (math.log(self.binsize) + F) - self.binsize * torch.exp(F) - torch.lgamma(Y + 1.0)

    def _ve_torch(self, f_means, f_vars, observations):
        y = observations
        return y * math.log(self.binsize) + y * f_means - self.binsize * torch.exp(f_means + 0.5 * f_vars) - torch.lgamma(y + 1.0)

    def predict_mean_and_var(self, f_means, f_vars):
        """Exact moments of y: m = b e^{mu + v/2}, m + (e^v - 1) m^2 (gpflow takes them by quadrature)."""
        m = self.binsize * torch.exp(f_means + 0.5 * f_vars)
        return m, m + torch.expm1(f_vars) * m * m


# ---- Power Expectation Propagation wrappers (markovflow/likelihoods/likelihoods.py:149-275), with the power applied ---------------------
class PEPScalarLikelihood:
    """A scalar likelihood `base` wrapped for Power Expectation Propagation: the tilted normaliser
        log Z = log int p(y | f)^alpha N(f; Fmu, Fvar) df
    and its first two derivatives with respect to Fmu (include/mfgm.h, mfgm_pep_tilted).  Unlike the reference, whose
    log_expected_density ignores alpha, the power is applied: with the exact power the EP fixed point of a Gaussian likelihood is its
    exact site for every alpha.

    `base` is Gaussian, Bernoulli, Poisson or any ScalarQuadratureLikelihood.  log Z is the n_gh-point Gauss-Hermite rule in log space
    (gpflow's quadrature.logspace), except for Bernoulli at alpha = 1, where it is the closed form the reference uses
    (base.predict_log_density).  The native route (one launch of mfgm_pep_tilted) runs when the base has a kind, the tensors are
    contiguous fp64 on the device, n_gh == 20 and nothing asks for a gradient; otherwise the torch route (the same formula, its
    derivatives by autograd twice, what the reference's nested GradientTape gives) runs, on any device.
    Shapes: Fmu, Fvar, Y [..., n, 1]; log Z [..., n]; d1, d2 [..., n, 1]."""

    def __init__(self, base, num_gauss_hermite_points=20):
        import numpy as np
        self.base = base
        self.num_gauss_hermite_points = self.n_gh = int(num_gauss_hermite_points)
        xi, w = np.polynomial.hermite.hermgauss(self.n_gh)
        self._xi, self._logw = xi, np.log(w / math.sqrt(math.pi))
        self._rule_cache = {}

    @property
    def kind(self):
        """mfgm_pep_tilted / mfgm_pep_sites kind of the native route, None when the base has none."""
        return getattr(self.base, "kind", None)

    @property
    def param(self):
        return self.base.param

    def _base_log_prob(self, F, Y):
        if isinstance(self.base, Gaussian):
            v = self.base.variance
            return -0.5 * math.log(2.0 * math.pi * v) - 0.5 * (Y - F) ** 2 / v
        return self.base.log_prob(F, Y)

    def _rule(self, like):
        key = str(like.device)
        r = self._rule_cache.get(key)
        if r is None:
            r = self._rule_cache[key] = (torch.tensor(self._xi, dtype=torch.float64, device=like.device),
                                         torch.tensor(self._logw, dtype=torch.float64, device=like.device))
        return r

    def _log_z_torch(self, Fmu, Fvar, Y, alpha):
        """log Z [..., n, 1] (differentiable)."""
        if isinstance(self.base, Bernoulli) and alpha == 1.0:
            x = Fmu / torch.sqrt(1.0 + Fvar)
            return torch.log(self.base._p(torch.where(Y == 1, x, -x)))
        xi, logw = self._rule(Fmu)
        X = Fmu[..., None] + math.sqrt(2.0) * torch.sqrt(Fvar)[..., None] * xi
        return torch.logsumexp(alpha * self._base_log_prob(X, Y[..., None]) + logw, dim=-1)

    def _native(self, Fmu, Fvar, Y):
        if self.kind is None or self.n_gh != 20 or not Fmu.is_cuda:
            return False
        ts = (Fmu, Fvar, Y)
        if any(t.requires_grad for t in ts) and torch.is_grad_enabled():
            return False
        return all(t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.shape == Fmu.shape for t in ts)

    def _launch(self, Fmu, Fvar, Y, alpha, want_grads):
        mk = lambda: torch.empty(Fmu.shape, dtype=torch.float64, device=Fmu.device)
        lz = mk()
        d1, d2 = (mk(), mk()) if want_grads else (None, None)
        _lib.check(_lib.load().mfgm_pep_tilted(self.kind, Fmu.numel(), _ptr(Fmu), _ptr(Fvar), _ptr(Y), float(self.param), float(alpha),
                                               _ptr(lz), _ptr(d1), _ptr(d2), _stream()), "mfgm_pep_tilted")
        return lz, d1, d2

    def log_expected_density(self, Fmu, Fvar, Y, alpha=1.0):
        """log int p(y = Y | f)^alpha N(f; Fmu, Fvar) df, [..., n]."""
        if self._native(Fmu, Fvar, Y):
            return self._launch(Fmu, Fvar, Y, alpha, False)[0][..., 0]
        return self._log_z_torch(Fmu, Fvar, Y, alpha)[..., 0]

    def grad_log_expected_density(self, Fmu, Fvar, Y, alpha=1.0):
        """(log Z [..., n], (d log Z / d Fmu, d^2 log Z / d Fmu^2) [..., n, 1] each)."""
        if self._native(Fmu, Fvar, Y):
            lz, d1, d2 = self._launch(Fmu, Fvar, Y, alpha, True)
            return lz[..., 0], (d1, d2)
        with torch.enable_grad():
            mu = Fmu.detach().requires_grad_(True)
            lz = self._log_z_torch(mu, Fvar.detach(), Y.detach(), alpha)
            (d1,) = torch.autograd.grad(lz.sum(), [mu], create_graph=True)
            (d2,) = torch.autograd.grad(d1.sum(), [mu])
        return lz.detach()[..., 0], (d1.detach(), d2)

    def predict_log_density(self, f_means, f_vars, observations):
        """The base likelihood's log predictive density, [..., n] (log N(y; mu, v + s^2) for a Gaussian base)."""
        if isinstance(self.base, Gaussian):
            v = f_vars + self.base.variance
            return (-0.5 * torch.log(2.0 * math.pi * v) - 0.5 * (observations - f_means) ** 2 / v).sum(-1)
        return self.base.predict_log_density(f_means, f_vars, observations)

    def predict_mean_and_var(self, f_means, f_vars):
        return self.base.predict_mean_and_var(f_means, f_vars)


class PEPGaussian(PEPScalarLikelihood):
    """The Gaussian likelihood N(y; f, s^2) with the tilted normaliser in closed form and the exact power:
        log Z = 1/2 (1 - alpha) log(2 pi s^2) - 1/2 log alpha + log N(y; Fmu, s^2/alpha + Fvar)
    (the reference's alpha log N(y; Fmu, s^2 + Fvar) is not this integral unless alpha = 1).  Native kind MFGM_LIK_GAUSSIAN."""

    def __init__(self, base):
        if not isinstance(base, Gaussian):
            raise TypeError("PEPGaussian wraps a Gaussian likelihood")
        super().__init__(base, num_gauss_hermite_points=20)

    @property
    def kind(self):
        from ._lib import LIK_GAUSSIAN
        return LIK_GAUSSIAN

    @property
    def param(self):
        return self.base.variance

    def _terms(self, Fmu, Fvar, Y, alpha):
        s2 = self.base.variance
        S = s2 / alpha + Fvar
        r = Y - Fmu
        lz = (0.5 * (1.0 - alpha) * math.log(2.0 * math.pi * s2) - 0.5 * math.log(alpha) - 0.5 * torch.log(2.0 * math.pi * S)
              - 0.5 * r * r / S)
        return lz, r / S, -1.0 / S

    def _log_z_torch(self, Fmu, Fvar, Y, alpha):
        return self._terms(Fmu, Fvar, Y, alpha)[0]

    def grad_log_expected_density(self, Fmu, Fvar, Y, alpha=1.0):
        if self._native(Fmu, Fvar, Y):
            return super().grad_log_expected_density(Fmu, Fvar, Y, alpha)
        lz, d1, d2 = self._terms(Fmu, Fvar, Y, alpha)
        return lz[..., 0], (d1, d2)


# ---- linear readout: a diffusion observed through f = H x + c with one scalar likelihood per output ------------------------------------
class LinearReadout:
    """p(y_i | x_i) = prod_j p_j(y_ij | f_ij),  f_ij = h_j^T x_i + c_j: the state of a diffusion model (CVISitesSSM, CVISitesSDE,
    CVISitesSDEQuadrature) seen through `emission` H [o, d] (1 <= o <= 8) and `offset` c [o] (default 0), with one scalar likelihood per
    output -- `likelihoods` is one likelihood shared by all outputs or a sequence of o of them.  A NaN entry of y says that the output was
    not observed there: it contributes exactly 0 to the variational expectation and to the gradients.

    Contract (include/mfgm.h, mfgm_readout), per observation with marginal N(mu, Sigma), m_j = h_j^T mu + c_j, v_j = h_j^T Sigma h_j and
    (ve_j, dm_j, dv_j) the scalar likelihood's variational expectation and its derivatives at (m_j, v_j):
        VE = sum_j ve_j,   g2 = sum_j dv_j h_j h_j^T,   g1 = sum_j h_j (dm_j - 2 dv_j h_j^T mu)
    (the gradient with respect to the expectation parameters of the state; the offset does not enter g1 through mu).

    Gaussian, Bernoulli and Poisson factors are the native kinds: the diffusion models then make the data-site update and the
    variational expectations in one HIP launch each (Plan.readout_site_update / readout_obs_ve).  The methods
    below are the torch route: any ScalarQuadratureLikelihood, any device, differentiable.  H and c are fixed (not trainable)."""

    uniform_site_gradient = False      # the site gradient depends on q: the models keep the dense per-node arrays

    def __init__(self, emission, likelihoods, offset=None):
        H = torch.as_tensor(emission, dtype=torch.float64).detach()
        if H.dim() != 2 or not 1 <= H.shape[0] <= 8:
            raise ValueError("emission must be [o, d] with 1 <= o <= 8")
        self.obs_dim, self.state_dim = int(H.shape[0]), int(H.shape[1])
        c = torch.zeros(self.obs_dim, dtype=torch.float64) if offset is None else torch.as_tensor(offset, dtype=torch.float64).detach()
        if tuple(c.shape) != (self.obs_dim,):
            raise ValueError("offset must be [o]")
        self.emission, self.offset = H.contiguous(), c.to(H.device).contiguous()
        if isinstance(likelihoods, (list, tuple)):
            if len(likelihoods) != self.obs_dim:
                raise ValueError("one likelihood per output (or a single shared one)")
            self.likelihoods = list(likelihoods)
        else:
            self.likelihoods = [likelihoods] * self.obs_dim
        for b in self.likelihoods:
            if not isinstance(b, (Gaussian, ScalarQuadratureLikelihood)):
                raise TypeError("the factors of a LinearReadout are Gaussian or ScalarQuadratureLikelihood (Bernoulli, Poisson, ...)")
        self._dev_cache, self._desc = {}, None

    # ---- native description ----------------------------------------------------------------------------------------------------------
    @property
    def native_kinds(self):
        """True when every factor is one of the kinds the HIP kernels know (Gaussian, Bernoulli, Poisson themselves, not subclasses)."""
        return all(type(b) in (Gaussian, Bernoulli, Poisson) for b in self.likelihoods) and self.state_dim <= 8

    def descriptor(self):
        """_lib.Readout of the emission, the offset and the factors' current parameters (native kinds only); rebuilt when a parameter
        has changed."""
        if not self.native_kinds:
            raise TypeError("a LinearReadout with a factor other than Gaussian, Bernoulli or Poisson (or d > 8) has no native description")
        key = tuple((type(b), b.variance if type(b) is Gaussian else b.param) for b in self.likelihoods)
        if self._desc is not None and self._desc[0] == key:
            return self._desc[1]
        rd = _lib.Readout()
        rd.o, rd.d = self.obs_dim, self.state_dim
        for j, b in enumerate(self.likelihoods):
            if type(b) is Gaussian:
                rd.kind[j], rd.param[j] = _lib.LIK_GAUSSIAN, b.variance
            else:
                rd.kind[j], rd.param[j] = b.kind, b.param
            rd.offset[j] = float(self.offset[j])
        for k, v in enumerate(self.emission.reshape(-1).tolist()):
            rd.H[k] = v
        self._desc = (key, rd)
        return rd

    def _Hc(self, like):
        """(H, c) on `like`'s device (made once per device)."""
        key = str(like.device)
        r = self._dev_cache.get(key)
        if r is None:
            r = self._dev_cache[key] = (self.emission.to(like.device), self.offset.to(like.device))
        return r

    # ---- projections -----------------------------------------------------------------------------------------------------------------
    def project(self, f_means, f_covariances):
        """(m, v) [..., n, o]: m_j = h_j^T mu + c_j, v_j = h_j^T Sigma h_j."""
        H, c = self._Hc(f_means)
        hm = (f_means[..., None, :] * H).sum(-1)
        v = ((f_covariances[..., None, :, :] * H[:, None, :]).sum(-1) * H).sum(-1)
        return hm + c, v

    @staticmethod
    def _seen(observations):
        """(mask of the observed entries, y with the others replaced by 0)."""
        seen = ~torch.isnan(observations)
        return seen, torch.where(seen, observations, torch.zeros_like(observations))

    def _per_output(self, fn, *cols):
        """fn(base_j, column j of every tensor as [..., n, 1]) for each output, stacked on a new last axis."""
        return torch.stack([fn(b, *(t[..., j:j + 1] for t in cols)) for j, b in enumerate(self.likelihoods)], dim=-1)

    # ---- interface of the diffusion models -----------------------------------------------------------------------------------------------
    def variational_expectations(self, f_means, f_covariances, observations):
        """E_q log p(y_i | x_i) = sum over the observed outputs of the factors' variational expectations, [..., n] (differentiable)."""
        m, v = self.project(f_means, f_covariances)
        seen, y = self._seen(observations)
        ve = self._per_output(lambda b, mj, vj, yj: b.variational_expectations(mj, vj, yj).reshape(mj.shape[:-1]), m, v, y)
        return torch.where(seen, ve, torch.zeros_like(ve)).sum(-1)

    @staticmethod
    def _scalar_derivatives(b, mj, vj, yj):
        """(dVE/dm, dVE/dv) [..., n, 1] of one factor."""
        if isinstance(b, Gaussian):
            return (yj - mj) / b.variance, torch.full_like(vj, -0.5 / b.variance)
        mj, vj, yj = mj.contiguous(), vj.contiguous(), yj.contiguous()
        if b._native(mj, vj, yj):
            _, g1, g2 = b._launch(mj, vj, yj, grads=True)      # (dm - 2 dv m, dv)
            return g1 + 2.0 * g2 * mj, g2
        with torch.enable_grad():
            mu = mj.detach().requires_grad_(True)
            var = vj.detach().requires_grad_(True)
            dm, dv = torch.autograd.grad(b._ve_torch(mu, var, yj.detach()).sum(), [mu, var])
        return dm, dv

    def ve_gradients_expectation(self, f_means, f_covariances, observations):
        """(g1 [..., n, d], g2 [..., n, d, d]): the gradient of sum_i VE_i with respect to the expectation parameters (mu, Sigma + mu mu^T)
        of the state."""
        H, c = self._Hc(f_means)
        f_means, f_covariances = f_means.detach(), f_covariances.detach()
        m, v = self.project(f_means, f_covariances)
        seen, y = self._seen(observations.detach())
        dm, dv = [], []
        for j, b in enumerate(self.likelihoods):
            a, e = self._scalar_derivatives(b, m[..., j:j + 1], v[..., j:j + 1], y[..., j:j + 1])
            dm.append(a[..., 0])
            dv.append(e[..., 0])
        zero = torch.zeros_like(m)
        dm, dv = torch.where(seen, torch.stack(dm, -1), zero), torch.where(seen, torch.stack(dv, -1), zero)
        a = dm - 2.0 * dv * (m - c)
        g1 = (a[..., :, None] * H).sum(-2)
        g2 = ((dv[..., :, None] * H)[..., :, :, None] * H[:, None, :]).sum(-3)
        return g1, g2

    # ---- predictions -------------------------------------------------------------------------------------------------------------------
    def predict_mean_and_var(self, f_means, f_covariances):
        """Mean and variance of every output, [..., n, o] each (per output the factor's predict_mean_and_var at (m_j, v_j))."""
        m, v = self.project(f_means, f_covariances)
        out = [b.predict_mean_and_var(m[..., j:j + 1], v[..., j:j + 1]) for j, b in enumerate(self.likelihoods)]
        return torch.cat([a for a, _ in out], -1), torch.cat([e for _, e in out], -1)

    def predict_log_density(self, f_means, f_covariances, observations):
        """log p(y_i) under the marginal, summed over the observed outputs, [..., n]: log N(y; m, v + s^2) for a Gaussian factor, the
        factor's own predict_log_density otherwise."""
        m, v = self.project(f_means, f_covariances)
        seen, y = self._seen(observations)

        def one(b, mj, vj, yj):
            if isinstance(b, Gaussian):
                s = vj + b.variance
                return (-0.5 * torch.log(2.0 * math.pi * s) - 0.5 * (yj - mj) ** 2 / s).sum(-1)
            return b.predict_log_density(mj, vj, yj)

        lp = self._per_output(one, m, v, y)
        return torch.where(seen, lp, torch.zeros_like(lp)).sum(-1)


# ---- multi-latent likelihoods (markovflow/likelihoods/mutlistage_likelihood.py; docs/notebooks/stacked_kernels.py) -------------------------
class _MultiLatentLikelihood:
    """A likelihood of one observation y that couples `latent_dim` latent values through the factorised marginals
    q(F) = prod_l N(F_l; Fmu_l, Fvar_l).  Fmu, Fvar [..., L], Y [..., 1]; variational_expectations [...]; the gradients with respect to
    the expectation parameters of every latent, g1_l = dVE/dm_l - 2 (dVE/dv_l) m_l and g2_l = dVE/dv_l, [..., L] each, in explicit
    form (for a quadrature term: the derivatives of the rule, as mfgm_scalar_lik defines them).  Plain torch on any device: the torch
    route of MultiLatentSparseCVI and the anchor of its kernels (include/mfgm.h, mfgm_ml_predict_lik)."""

    latent_dim = None
    ml_kind = None          # mfgm_ml_lik kind of the native route

    @property
    def ml_params(self):
        return (0.0, 0.0)

    def _ve_and_derivatives(self, Fmu, Fvar, Y):
        """(VE [...], dVE/dm [..., L], dVE/dv [..., L])."""
        raise NotImplementedError

    def variational_expectations(self, Fmu, Fvar, Y):
        return self._ve_and_derivatives(Fmu, Fvar, Y)[0]

    def ve_gradients_expectation(self, Fmu, Fvar, Y):
        _, dm, dv = self._ve_and_derivatives(Fmu.detach(), Fvar.detach(), Y.detach())
        return dm - 2.0 * dv * Fmu.detach(), dv

    def predict_log_density(self, Fmu, Fvar, Y):
        raise NotImplementedError(f"{type(self).__name__} has no predictive density (as in the reference)")

    def predict_mean_and_var(self, Fmu, Fvar):
        raise NotImplementedError(f"{type(self).__name__} has no predictive moments (as in the reference)")


class MultiStageLikelihood(_MultiLatentLikelihood):
    """markovflow/likelihoods/mutlistage_likelihood.py: intermittent-demand counts through a decision tree of three latents,
        y == 0:  log p = B+(F0);     y == 1:  log p = B-(F0) + B+(F1);     y >= 2:  log p = B-(F0) + B-(F1) + Pois(y - 2; F2)
    with B+- the jittered-probit Bernoulli log-probability of label 1 / 0 (Bernoulli above) and Pois the exp-link Poisson with bin size
    `binsize` (Poisson above).  Any other y (negative, NaN, non-integer below 2) contributes zero to everything, as the reference's
    where-chain.  The variational expectation applies the same cases to the per-latent expectations: the 20-point Gauss-Hermite rule
    for the Bernoulli terms, the closed form for the Poisson term; a latent outside a point's case has zero gradients there."""

    latent_dim = 3
    ml_kind = _lib.ML_MULTISTAGE

    def __init__(self, jitter=1e-3, binsize=1.0):
        import numpy as np
        self.jitter, self.binsize = float(jitter), float(binsize)
        if not 0.0 <= self.jitter < 0.5:
            raise ValueError("jitter must lie in [0, 1/2)")
        if not (self.binsize > 0.0 and math.isfinite(self.binsize)):
            raise ValueError("binsize must be positive")
        xi, w = np.polynomial.hermite.hermgauss(20)
        self._xi, self._w = xi, w / math.sqrt(math.pi)
        self._rule_cache = {}

    @property
    def ml_params(self):
        return (self.jitter, self.binsize)

    def _rule(self, like):
        key = str(like.device)
        r = self._rule_cache.get(key)
        if r is None:
            r = self._rule_cache[key] = (torch.tensor(self._xi, dtype=torch.float64, device=like.device),
                                         torch.tensor(self._w, dtype=torch.float64, device=like.device))
        return r

    def _p(self, f):
        return self.jitter + (1.0 - 2.0 * self.jitter) * _probit(f)

    def _bernoulli_rule(self, mu, v, s):
        """(VE, dVE/dmu, dVE/dv) of log p_j(s F) under N(mu, v) by the 20-point rule; s = +1 for label 1, -1 for label 0."""
        xi, w = self._rule(mu)
        sc = math.sqrt(2.0) * torch.sqrt(v)
        X = mu[..., None] + sc[..., None] * xi
        p = self._p(s[..., None] * X)
        dl = s[..., None] * (1.0 - 2.0 * self.jitter) * torch.exp(-0.5 * X * X) * (1.0 / math.sqrt(2.0 * math.pi)) / p
        return (w * torch.log(p)).sum(-1), (w * dl).sum(-1), (w * dl * xi).sum(-1) / sc

    @staticmethod
    def _cases(Y):
        y = Y[..., 0]
        return y == 0, y == 1, y >= 2

    def _ve_and_derivatives(self, Fmu, Fvar, Y):
        is0, is1, big = self._cases(Y)
        one = torch.ones_like(Fmu[..., 0])
        zero = torch.zeros_like(one)
        ve0, a0, e0 = self._bernoulli_rule(Fmu[..., 0], Fvar[..., 0], torch.where(is0, one, -one))
        ve1, a1, e1 = self._bernoulli_rule(Fmu[..., 1], Fvar[..., 1], torch.where(is1, one, -one))
        cnt = torch.where(big, Y[..., 0] - 2.0, zero)
        rate = self.binsize * torch.exp(Fmu[..., 2] + 0.5 * Fvar[..., 2])
        ve2 = cnt * math.log(self.binsize) + cnt * Fmu[..., 2] - rate - torch.lgamma(cnt + 1.0)
        in0, in1 = is0 | is1 | big, is1 | big
        ve = torch.where(in0, ve0, zero) + torch.where(in1, ve1, zero) + torch.where(big, ve2, zero)
        dm = torch.stack([torch.where(in0, a0, zero), torch.where(in1, a1, zero), torch.where(big, cnt - rate, zero)], -1)
        dv = torch.stack([torch.where(in0, e0, zero), torch.where(in1, e1, zero), torch.where(big, -0.5 * rate, zero)], -1)
        return ve, dm, dv

    def log_prob(self, F, Y):
        """log p(y | F), [...]."""
        is0, is1, big = self._cases(Y)
        zero = torch.zeros_like(F[..., 0])
        cnt = torch.where(big, Y[..., 0] - 2.0, zero)
        lp0, ln0 = torch.log(self._p(F[..., 0])), torch.log(self._p(-F[..., 0]))
        lp1, ln1 = torch.log(self._p(F[..., 1])), torch.log(self._p(-F[..., 1]))
        lp2 = cnt * (math.log(self.binsize) + F[..., 2]) - self.binsize * torch.exp(F[..., 2]) - torch.lgamma(cnt + 1.0)
        return torch.where(is0, lp0, zero) + torch.where(is1, ln0 + lp1, zero) + torch.where(big, ln0 + ln1 + lp2, zero)

    def sample_y(self, F, seed=0):
        """y [..., 1] drawn from p(y | F) down the tree: y = 0 with probability p_j(F0), else 1 with probability p_j(F1), else
        2 + Poisson(binsize e^{F2}) (sample_y of the reference, on a torch generator seeded with `seed`)."""
        gen = torch.Generator(device=F.device)
        gen.manual_seed(int(seed))
        eta0 = torch.bernoulli(self._p(F[..., 0]), generator=gen)
        eta1 = torch.bernoulli(self._p(F[..., 1]), generator=gen)
        lam = torch.poisson(self.binsize * torch.exp(F[..., 2]), generator=gen)
        y = torch.where((eta0 == 0) & (eta1 == 1), torch.ones_like(lam), torch.zeros_like(lam))
        return (y + torch.where((eta0 == 0) & (eta1 == 0), lam + 2.0, torch.zeros_like(lam)))[..., None]


class HeteroskedasticGaussian(_MultiLatentLikelihood):
    """y ~ N(F0, exp F1): one latent for the mean and one for the log-variance (docs/notebooks/stacked_kernels.py of the reference).
    VE = -1/2 [log 2 pi + m1 + exp(-m1 + v1 / 2) ((m0 - y)^2 + v0)] in closed form; dVE/dv_l <= 0 for both latents at every input, so
    the posterior precision stays positive definite."""

    latent_dim = 2
    ml_kind = _lib.ML_HETGAUSS

    def _ve_and_derivatives(self, Fmu, Fvar, Y):
        m0, m1, v0, v1 = Fmu[..., 0], Fmu[..., 1], Fvar[..., 0], Fvar[..., 1]
        s = torch.exp(-m1 + 0.5 * v1)
        r = m0 - Y[..., 0]
        q = r * r + v0
        ve = -0.5 * (math.log(2.0 * math.pi) + m1 + s * q)
        return ve, torch.stack([-s * r, -0.5 + 0.5 * s * q], -1), torch.stack([-0.5 * s, -0.25 * s * q], -1)

    def log_prob(self, F, Y):
        return -0.5 * (math.log(2.0 * math.pi) + F[..., 1] + torch.exp(-F[..., 1]) * (Y[..., 0] - F[..., 0]) ** 2)

    def sample_y(self, F, seed=0):
        gen = torch.Generator(device=F.device)
        gen.manual_seed(int(seed))
        eps = torch.randn(F.shape[:-1], dtype=F.dtype, device=F.device, generator=gen)
        return (F[..., 0] + torch.exp(0.5 * F[..., 1]) * eps)[..., None]
