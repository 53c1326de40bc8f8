"""
Power Expectation Propagation on the sites-on-f GP model (markovflow/models/pep.py, `PowerExpectationPropagation`,
`gradient_correction`): one scalar Gaussian site t_n(f_n) = exp(eta1 f + eta2 f^2) per data point, updated against the cavity
q(f) / t_n(f_n)^alpha and the tilted distribution p(y_n | f_n)^alpha x cavity.  The per-point update runs in one HIP launch
(mfgm_pep_sites, include/mfgm.h) on the f-marginals of the fused predict (mfgm_kf_sites_predict).  DESIGN.md section 13.

Two deliberate differences from the reference: the power alpha is applied to the likelihood inside the tilted normaliser (the
reference's likelihood wrappers ignore it or scale the log density instead), and the energy's per-point terms are taken at the cavity,
as the site update takes them (the reference's compute_log_norm evaluates them at the posterior marginal).  Points whose cavity is not
a proper Gaussian keep their sites and are counted in `skipped` (the reference produces NaN there).
"""
import math

import numpy as np
import torch

from . import _lib, linalg
from .packed import _ptr, _stream
from .stamps import wrote
from .variational_cvi import GaussianProcessWithSitesBase, back_project_nats


def gradient_correction(inputs, grads):
    """(L1, L2) = (2 L2 (g1/g2 - i1), 1/2 / (i2 + 1/g2)) for inputs (i1, i2) = (cavity mean, cavity variance) and grads (g1, g2) = the
    first two derivatives of log Z with respect to the cavity mean (pep.py:250-261): the natural parameters of the moment-matched site."""
    L2 = 0.5 / (inputs[1] + 1.0 / grads[1])
    L1 = 2.0 * L2 * (grads[0] / grads[1] - inputs[0])
    return L1, L2


def _log_norm_1d(m, v):
    """n(m, v) = 1/2 (log v + m^2 / v): log normaliser of a univariate Gaussian in natural form, up to 1/2 log 2 pi."""
    return 0.5 * (torch.log(v) + m * m / v)


class PowerExpectationPropagation(GaussianProcessWithSitesBase):
    """pep.py:28-247.  One chain: time points [N], observations [N, 1]."""

    def __init__(self, input_data, kernel, likelihood, mean_function=None, learning_rate=1.0, alpha=1.0):
        # mean_function is the reference's signature only here: PEP's sites are on f itself and the model has never used it
        super().__init__(input_data, kernel, likelihood, None)
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError("alpha must lie in (0, 1]")
        if not 0.0 <= float(learning_rate) <= 1.0:
            raise ValueError("learning_rate must lie in [0, 1]")
        if self._time_points.dim() != 1:
            raise NotImplementedError("PowerExpectationPropagation runs one chain: time points [N], observations [N, 1]")
        self.learning_rate = float(learning_rate)
        self.alpha = float(alpha)
        y = self._observations
        # site log normalisers start at zero (variational_cvi.py:99-103 of the reference)
        self.sites.log_norm = torch.zeros_like(y)
        # points whose update was skipped (improper cavity or non-finite moments), accumulated on the device
        self.skipped = torch.zeros(1, dtype=torch.int32, device=y.device)
        self._norm_p = None

    @property
    def num_data(self):
        return int(self._observations.shape[0])

    # ---- reference interface ------------------------------------------------------------------------------------------------------
    def local_objective(self, Fmu, Fvar, Y):
        """log E_q(f) p(y | f)^alpha (pep.py:93-95)."""
        return self._likelihood.log_expected_density(Fmu, Fvar, Y, alpha=self.alpha)

    def local_objective_gradients(self, Fmu, Fvar):
        """(log Z, gradient_correction([Fmu, Fvar], (d1, d2))) (pep.py:97-103)."""
        obj, grads = self._likelihood.grad_log_expected_density(Fmu, Fvar, self._observations, alpha=self.alpha)
        return obj, gradient_correction([Fmu, Fvar], grads)

    def _site_index(self, site_indices):
        """(int64 device tensor of distinct indices, count), or (None, N) for every site.  Accepts [k, 1] (the reference's shape) or [k];
        duplicates count once; out-of-range indices raise ValueError.  Validated on the host (the one synchronisation of update_sites,
        and only when indices are given)."""
        n = self.num_data
        if site_indices is None:
            return None, n
        arr = site_indices.detach().cpu().numpy() if torch.is_tensor(site_indices) else np.asarray(site_indices)
        if arr.ndim == 2 and arr.shape[1] == 1:
            arr = arr[:, 0]
        if arr.ndim != 1:
            raise ValueError("site_indices must have shape [k, 1] or [k]")
        if arr.size and not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("site_indices must be integers")
        arr = np.unique(arr.astype(np.int64))
        if arr.size and (arr[0] < 0 or arr[-1] >= n):
            raise ValueError(f"site_indices out of range [0, {n})")
        return torch.as_tensor(arr, dtype=torch.int64, device=self._observations.device), int(arr.size)

    def mask_indices(self, exclude_indices):
        """Float mask [N]: 1 at the given indices, 0 elsewhere.  None selects every site (the reference returns zeros there, so that its
        update_sites() without indices changes nothing)."""
        y = self._observations
        if exclude_indices is None:
            return torch.ones(y.shape[:1], dtype=y.dtype, device=y.device)
        idx, _ = self._site_index(exclude_indices)
        return torch.zeros(y.shape[:1], dtype=y.dtype, device=y.device).index_fill_(0, idx, 1.0)

    def compute_cavity_from_marginals(self, marginals):
        """f-marginals of the cavities from the state marginals (means [N, d], covs [N, d, d]), in the reference's state-space form
        (pep.py:115-147): posterior naturals per state minus alpha times the back-projected site, then projected onto f."""
        means, covs = marginals
        d = covs.shape[-1]
        eye = torch.eye(d, dtype=covs.dtype, device=covs.device).expand(covs.shape).contiguous()
        chol = linalg.cholesky(covs)
        nat2 = -0.5 * linalg.cholesky_solve(eye, chol)
        nat1 = linalg.cholesky_solve(means[..., None].contiguous(), chol)[..., 0]
        em = self._emission()
        bp1, bp2 = back_project_nats(self.sites.nat1, self.sites.nat2[..., 0], em.emission_matrix)
        cav_nat2 = nat2 - bp2 * self.alpha
        cav_nat1 = nat1 - bp1 * self.alpha
        cav_chol = linalg.cholesky((-cav_nat2).contiguous())
        cav_means = 0.5 * linalg.cholesky_solve(cav_nat1[..., None].contiguous(), cav_chol)[..., 0]
        cav_covs = 0.5 * linalg.cholesky_solve(eye, cav_chol)
        return em.project_state_to_f(cav_means), em.project_state_covariance_to_f(cav_covs, full_output_cov=False)

    def compute_cavity(self):
        """Cavity f-marginals q^{-n}(f_n) of q(f) / t_n(f_n)^alpha at every data point (pep.py:149-157)."""
        return self.compute_cavity_from_marginals(self.dist_q.marginals)

    def _cavity_f(self, fmu, fvar):
        """The same cavities from the f-marginals (the rank-one cavity of the state projected onto f): (mc, vc, lc)."""
        lc = 1.0 / fvar + 2.0 * self.alpha * self.sites.nat2[..., 0]
        vc = 1.0 / lc
        return vc * (fmu / fvar - self.alpha * self.sites.nat1), vc, lc

    def _native(self, fmu, fvar):
        lik = self._likelihood
        ts = (fmu, fvar, self._observations, self.sites.nat1, self.sites.nat2, self.sites.log_norm)
        return (getattr(lik, "kind", None) is not None and getattr(lik, "n_gh", 20) == 20
                and all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() for t in ts) and fmu.numel() == self.num_data)

    def _launch(self, fmu, fvar, lr, idx, k, lnorm, e_out, skipped):
        lik, s = self._likelihood, self.sites
        _lib.check(_lib.load().mfgm_pep_sites(lik.kind, self.num_data, _ptr(fmu), _ptr(fvar), _ptr(self._observations), float(lik.param),
                                              self.alpha, float(lr), _ptr(idx), k, _ptr(s.nat1), _ptr(s.nat2), _ptr(lnorm), _ptr(e_out),
                                              _ptr(skipped), _stream()), "mfgm_pep_sites")

    def compute_log_norm(self):
        """Per-point energy terms e_n = log Z_n + n(cavity) - n(marginal), [N], with log Z_n taken at the cavity (the reference takes
        it at the posterior marginal, pep.py:159-177, which is not the EP energy)."""
        fmu, fvar = self.predict_f_at_data()
        if self._native(fmu, fvar):
            e = torch.empty_like(fmu)
            self._launch(fmu, fvar, 0.0, None, self.num_data, None, e, None)
            return e[..., 0]
        mc, vc, _ = self._cavity_f(fmu, fvar)
        lz = self._likelihood.log_expected_density(mc, vc, self._observations, alpha=self.alpha)
        return lz + (_log_norm_1d(mc, vc) - _log_norm_1d(fmu, fvar))[..., 0]

    def update_sites(self, site_indices=None):
        """One damped PEP update of the given sites (all when None) (pep.py:179-215): site <- (1 - lr) site + lr ((1 - alpha) site +
        moment-matched site), log_norm likewise with the energy term."""
        fmu, fvar = self.predict_f_at_data()
        idx, k = self._site_index(site_indices)
        if k == 0:
            return
        s = self.sites
        if self._native(fmu, fvar):
            self._launch(fmu, fvar, self.learning_rate, idx, k, s.log_norm, None, self.skipped)
            wrote(s.nat1, s.nat2, s.log_norm)
            return
        # torch route (a likelihood without a kind): the same update, element-wise
        a, lr = self.alpha, self.learning_rate
        mc, vc, lc = self._cavity_f(fmu, fvar)
        lz, grads = self._likelihood.grad_log_expected_density(mc, vc, self._observations, alpha=a)
        L1, L2 = gradient_correction([mc, vc], grads)
        e = lz[..., None] + _log_norm_1d(mc, vc) - _log_norm_1d(fmu, fvar)
        n2 = s.nat2[..., 0]
        new1 = (1 - lr) * s.nat1 + lr * ((1 - a) * s.nat1 + L1)
        new2 = (1 - lr) * n2 + lr * ((1 - a) * n2 + L2)
        new3 = (1 - lr) * s.log_norm + lr * ((1 - a) * s.log_norm + e)
        ok = (fvar > 0) & (lc > 0) & torch.isfinite(L1) & torch.isfinite(L2)
        sel = self.mask_indices(None).bool()[:, None] if idx is None else torch.zeros_like(ok).index_fill_(0, idx, True)
        upd = sel & ok
        self.skipped += (sel & ~ok).sum().to(torch.int32)
        s.nat1.copy_(torch.where(upd, new1, s.nat1))
        s.nat2.copy_(torch.where(upd, new2, n2)[..., None])
        s.log_norm.copy_(torch.where(upd, new3, s.log_norm))

    @property
    def num_skipped(self):
        """Host count of skipped site updates so far (synchronises)."""
        return int(self.skipped.item())

    def _dist_p_normalizer(self):
        if self._norm_p is None:                     # the prior is fixed
            self._norm_p = self.dist_p.normalizer()
        return self._norm_p

    def _dist_q_normalizer(self):
        """dist_q.normalizer() without building dist_q: the posterior precision Lambda and Lambda mu are the posterior naturals, so one
        factorisation of them gives log det Lambda and |L^T mu|^2."""
        pl, lin, diag, sub = self._posterior_naturals()
        f = pl.factor(diag, sub, lin, aD=-2.0, aS=-1.0, aR=1.0, want_logdet=True, want_quad=True, store_G=pl.wide)
        ssm = self.dist_p
        return (0.5 * float(ssm.T * ssm.d) * math.log(2.0 * math.pi) - f["logdet"] + 0.5 * f["quad"]).reshape(ssm.batch_shape)

    def energy(self):
        """PEP energy  dist_q.normalizer() - dist_p.normalizer() + 1/alpha sum_n e_n  (pep.py:223-230, e_n at the cavity); a device
        scalar.  At the fixed point of a Gaussian likelihood it is the exact log marginal likelihood for every alpha."""
        return self._dist_q_normalizer() - self._dist_p_normalizer() + self.compute_log_norm().sum() / self.alpha

    def kernel_changed(self):
        super().kernel_changed()
        self._norm_p = None

    def _step_sites(self):
        return self.sites.nat1, self.sites.nat2, self.sites.log_norm
