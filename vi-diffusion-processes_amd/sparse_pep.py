"""
Sparse Power Expectation Propagation (markovflow/models/sparse_pep.py, `SparsePowerExpectationPropagation`): M + 1 Gaussian sites
t_m(v_m) = exp(nat1_m^T v + v^T nat2_m v) on the pairs v_m of consecutive inducing states, updated against the cavity
q(v_m) / t_m(v_m)^(alpha / n_m) and the tilted distributions of the n_m data points of interval m.  Every point of an interval removes
the same fraction of the same site, so the cavity is computed once per INTERVAL (two [2d, 2d] factorisations per interval); the whole
update is one launch of mfgm_sparse_pep_sites[_q] (include/mfgm.h, csrc/mfgm_spep.h) on the cached posterior marginals of
SparseCVIGaussianProcess.  DESIGN.md section 14.

Three deliberate differences from the reference:
1. The cavity variance `s` in L2 = 1/2 / (s + 1/d2) excludes the conditional variance c_i (the reference hands fx_covs, which includes
   it, to gradient_correction).  With s this is exact moment matching on v_m: a Gaussian likelihood's site is
   N(y_i; w_i^T v, sigma^2 / alpha + c_i) whatever the cavity.  The two agree where c_i = 0 (inducing points on the data).
2. The normaliser ratio G(cavity) - G(q) is taken from the PAIR marginal, g_c - g_q: the removed factor depends on v_m only, so
   Z_cav / Z_q = E_q[t_m(v_m)^(-beta)] is a 2d-dimensional Gaussian integral -- an identity, in place of the reference's M + 1 chain
   normalisers.
3. The energy terms e_i are taken at the cavity and in the same pass as the site update (the reference updates the sites first and
   recomputes); the update adds sum_i dX_i to (1 - alpha) X_m (the dense model's form) where the reference writes alpha * sum.
As in pep.py the power alpha is applied to the likelihood inside the tilted normaliser, and intervals whose cavity is not a proper
Gaussian keep their sites and are counted in `skipped`.

With several points per interval the points share one tied site (the reference's `fraction_sites`), so the fixed point under a
non-Gaussian likelihood is that of tied-site Power EP.
"""
import ctypes
import math

import torch

from . import _lib
from .conditionals import _cond_stats, base_conditional_predict
from .packed import _ptr, _stream
from .pair_sites import dense_posterior, dense_prior, on_device
from .pep import gradient_correction
from .sparse_variational_cvi import DenseRouteSparseCVI
from .stamps import wrote


def _chol_parts(A):
    """(ok [B], L^-1 [B, n, n], sum log diag L [B]) of a batch of symmetric matrices; members that are not positive definite are
    replaced by the identity and reported in ok."""
    L, info = torch.linalg.cholesky_ex(A)
    ok = (info == 0) & torch.isfinite(A).all(-1).all(-1)
    eye = torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
    L = torch.where(ok[:, None, None], L, eye)
    Li = torch.linalg.solve_triangular(L, eye.expand_as(L), upper=False)
    return ok, Li, torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)


def interval_update(likelihood, alpha, lr, idx, w, c, y, mu, S, nat1, nat2, lnorm):
    """The per-interval update in batched [M + 1, 2d, 2d] torch operations (the torch route; the algorithm of mfgm_sparse_pep_sites):
    idx [N] interval of each point, w [N, 2d], c [N], y [N], pair marginals mu [M+1, 2d], S [M+1, 2d, 2d], sites nat1 / nat2 /
    lnorm [M+1].  Returns (nat1, nat2, lnorm, e [M+1], skipped)."""
    M1 = mu.shape[0]
    cnt = torch.bincount(idx, minlength=M1)
    has = cnt > 0
    beta = alpha / cnt.clamp_min(1).to(mu.dtype)
    ok_s, Li, ldS = _chol_parts(S)
    u = (Li @ mu[..., None])[..., 0]
    h = (Li.transpose(-1, -2) @ u[..., None])[..., 0]
    gq = ldS + 0.5 * (u * u).sum(-1)
    Lam = Li.transpose(-1, -2) @ Li
    ok_c, Lci, ldC = _chol_parts(Lam + 2.0 * beta[:, None, None] * nat2)
    uc = (Lci @ (h - beta[:, None] * nat1)[..., None])[..., 0]
    gc = -ldC + 0.5 * (uc * uc).sum(-1)
    ok = (ok_s & ok_c) | ~has
    # the points grouped by interval; the k-th point of every interval that has one at a time: no [N, 2d, 2d] gather
    order = torch.argsort(idx, stable=True)
    seg = torch.cumsum(cnt, 0) - cnt
    N = idx.numel()
    s, mc = torch.zeros(N, dtype=mu.dtype, device=mu.device), torch.zeros(N, dtype=mu.dtype, device=mu.device)
    kmax = int(cnt.max()) if N else 0
    groups = []
    for k in range(kmax):
        sel = torch.nonzero(cnt > k)[:, 0]
        i = order[seg[sel] + k]
        t = (Lci[sel] @ w[i][..., None])[..., 0]
        s[i] = (t * t).sum(-1)
        mc[i] = (t * uc[sel]).sum(-1)
        groups.append((sel, i))
    lz, (d1, d2) = likelihood.grad_log_expected_density(mc[:, None], (s + c)[:, None], y.reshape(-1, 1), alpha=alpha)
    L1, L2 = gradient_correction([mc, s], (d1[:, 0], d2[:, 0]))
    fin = torch.isfinite(L1) & torch.isfinite(L2)
    zero = torch.zeros_like(L1)
    L1, L2 = torch.where(fin, L1, zero), torch.where(fin, L2, zero)
    e = torch.zeros(M1, dtype=mu.dtype, device=mu.device).index_add_(0, idx, torch.where(fin, lz + (gc - gq)[idx], zero))
    d1s = torch.zeros_like(nat1).index_add_(0, idx, L1[:, None] * w)
    d2s = torch.zeros_like(nat2)
    for sel, i in groups:
        d2s[sel] += L2[i, None, None] * w[i][:, :, None] * w[i][:, None, :]
    new = [(1 - lr) * X + lr * ((1 - alpha) * X + dX) for X, dX in ((nat1, d1s), (nat2, d2s), (lnorm, e))]
    skipped = (cnt * ~ok).sum() + (~fin & ok[idx]).sum()
    return (torch.where(ok[:, None], new[0], nat1), torch.where(ok[:, None, None], new[1], nat2), torch.where(ok, new[2], lnorm),
            torch.where(ok, e, torch.full_like(e, float("nan"))), skipped.to(torch.int32))


class SparsePowerExpectationPropagation(DenseRouteSparseCVI):
    """sparse_pep.py:41-559.  One chain: inducing points [M]; sites nat1 [M+1, 2d], nat2 [M+1, 2d, 2d], log_norm [M+1, 1].
    The sites are public and assignable; every nat2_m must be symmetric (the kernel reads its lower triangle, the torch route the whole
    matrix).  `mean_function` is accepted for the reference's signature and ignored here (SparseCVIGaussianProcess itself applies it).
    `likelihood` is a PEP wrapper (PEPScalarLikelihood / PEPGaussian); classic_elbo and predict_log_density use the likelihood it wraps.
    On CPU tensors the posterior comes from a dense (M d) x (M d) inverse (pair_sites.py): that route exists for small models and the
    host tests only."""

    def __init__(self, kernel, inducing_points, likelihood, mean_function=None, learning_rate=1.0, alpha=1.0):
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError("alpha must lie in (0, 1]")
        if not 0.0 <= float(learning_rate) <= 1.0:
            raise ValueError("learning_rate must lie in [0, 1]")
        if inducing_points.dim() != 1:
            raise NotImplementedError("SparsePowerExpectationPropagation runs one chain: inducing points [M]")
        if inducing_points.shape[0] < 2:
            raise ValueError("at least two inducing points are needed")
        from .kernels import PiecewiseKernel
        if isinstance(kernel, PiecewiseKernel):
            raise NotImplementedError("SparsePowerExpectationPropagation does not take a PiecewiseKernel: its pair priors assume one "
                                      "stationary kernel on the whole axis")
        # the parent's objectives (classic_elbo, predict_log_density) take variational expectations: they get the wrapped likelihood
        base = likelihood if hasattr(likelihood, "variational_expectations") else likelihood.base
        super().__init__(kernel, inducing_points, base, None, float(learning_rate))
        self._pep = likelihood
        self.alpha = float(alpha)
        M, n = inducing_points.shape[0], 2 * kernel.state_dim
        dev = inducing_points.device
        self.nat2 = (-1e-10 * torch.eye(n, dtype=torch.float64, device=dev)).repeat(M + 1, 1, 1)
        self.log_norm = torch.zeros((M + 1, 1), dtype=torch.float64, device=dev)
        # data points whose update was skipped (improper cavity of their interval or non-finite moments), accumulated on the device
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        self._norm_p = None

    @property
    def likelihood(self):
        return self._pep

    @property
    def num_skipped(self):
        """Host count of skipped data points so far (synchronises)."""
        return int(self.skipped.item())

    # ---- counting (sparse_pep.py:176-195, 450-471) -----------------------------------------------------------------------------------
    def _indices(self, time_points):
        return torch.searchsorted(self.inducing_inputs.contiguous(), time_points.contiguous())

    def compute_num_data_per_interval(self, time_points):
        """n_m [M + 1] as floats."""
        return torch.bincount(self._indices(time_points).reshape(-1), minlength=self.inducing_inputs.shape[0] + 1).to(torch.float64)

    def fraction_sites(self, time_points):
        """1 / n_m, or 0 where n_m = 0, [M + 1]."""
        n = self.compute_num_data_per_interval(time_points)
        return torch.where(n > 0, 1.0 / n.clamp_min(1.0), torch.zeros_like(n))

    def compute_fraction(self, time_points):
        """The fraction of its interval's site that each data point owns, [N]."""
        return self.fraction_sites(time_points)[self._indices(time_points)]

    # ---- posterior ------------------------------------------------------------------------------------------------------------------
    def compute_posterior_ssm(self, nat1, nat2):
        """The posterior over the inducing states for the given sites, as a StateSpaceModel (sparse_pep.py:197-231)."""
        if not on_device(self):
            raise NotImplementedError("the posterior state-space model needs the sites on the device")
        return self._posterior_ssm(nat1.contiguous(), nat2.contiguous())

    def compute_marginals(self):
        """Pairwise marginals (means [M+1, 2d], covariances [M+1, 2d, 2d]) of the posterior, the prior's initial state at both ends
        (sparse_pep.py:240-249)."""
        return self._pair_marginals()

    # ---- the reference's per-point inspection helpers (they gather) ------------------------------------------------------------------
    def remove_cavity_from_marginals(self, time_points, marginals):
        """State marginals (means [N, d], covariances [N, d, d]) at the time points under the cavity of each point's interval
        (sparse_pep.py:251-293)."""
        pw_means, pw_covs = marginals
        n = pw_means.shape[-1]
        eye = torch.eye(n, dtype=torch.float64, device=pw_means.device)
        pw_prec = torch.linalg.inv(pw_covs)
        idx = self._indices(time_points)
        frac = self.compute_fraction(time_points) * self.alpha
        cav_prec = pw_prec[idx] + 2.0 * frac[:, None, None] * self.nat2[idx]
        cav_nat1 = (pw_prec @ pw_means[..., None])[..., 0][idx] - frac[:, None] * self.nat1[idx]
        cav_covs = torch.linalg.solve(cav_prec, eye.expand_as(cav_prec))
        cav_means = (cav_covs @ cav_nat1[..., None])[..., 0]
        P, T, _ = _cond_stats(time_points, self.inducing_inputs, self._kernel)
        return base_conditional_predict(P, T, cav_means, pairwise_state_covariances=cav_covs)

    def compute_cavity_state(self, time_points):
        return self.remove_cavity_from_marginals(time_points, self.compute_marginals())

    def compute_cavity(self, time_points):
        """Cavity marginals of f at the time points (sparse_pep.py:304-314), [N, 1] each."""
        sx_mus, sx_covs = self.compute_cavity_state(time_points)
        em = self._kernel.generate_emission_model(time_points)
        return em.project_state_to_f(sx_mus), em.project_state_covariance_to_f(sx_covs, full_output_cov=False)

    # ---- the update -----------------------------------------------------------------------------------------------------------------
    def _native(self, data):
        lik = self._pep
        if data is None or self._shard is not None or getattr(lik, "kind", None) is None or getattr(lik, "n_gh", 20) != 20:
            return False
        self._sync_sites()
        return (self._nat1.is_contiguous() and (self._packed or self._nat2.is_contiguous()) and self.log_norm.is_contiguous()
                and self.skipped.is_cuda)

    def _launch(self, data, observations, lr, lnorm, e_out, skipped):
        m = self._marginals()
        self._sync_sites()
        lik = self._pep
        y = self._own_observations(data, observations).reshape(-1).contiguous()
        fn, n2 = ((_lib.load().mfgm_sparse_pep_sites_q, self._nat2q) if self._packed
                  else (_lib.load().mfgm_sparse_pep_sites, self._nat2))
        _lib.check(fn(ctypes.byref(data["struct"]), lik.kind, _ptr(y), float(lik.param), self.alpha, float(lr), _ptr(m["mu"]),
                      _ptr(m["Sig"]), _ptr(m["Sub"]), _ptr(self._nat1), _ptr(n2), _ptr(lnorm), _ptr(e_out), _ptr(skipped), _stream()),
                   "mfgm_sparse_pep_sites")

    def _torch_terms(self, input_data):
        """(idx, w, c, y) of the torch route: any time points (flattened), any device."""
        time_points, observations = input_data
        t = time_points.reshape(-1)
        P, Tc, idx = _cond_stats(t, self.inducing_inputs, self._kernel)
        H = self._kernel.generate_emission_model(t[:1]).emission_matrix[0]
        return idx, (H @ P)[:, 0, :], (H @ Tc @ H.transpose(-1, -2))[:, 0, 0], observations.reshape(-1)

    def _torch_update(self, input_data, lr):
        idx, w, c, y = self._torch_terms(input_data)
        mu, S = self.compute_marginals()
        return interval_update(self._pep, self.alpha, lr, idx, w, c, y, mu, S, self.nat1, self.nat2, self.log_norm[:, 0])

    def compute_new_sites(self, input_data):
        """(nat1, nat2) after one damped update, the model left as it is (sparse_pep.py:316-380)."""
        n1, n2, _, _, _ = self._torch_update(input_data, self.learning_rate)
        return n1, n2

    def compute_log_norm(self, input_data):
        """sum_{i in m} e_i per interval, [M + 1]: e_i = log Z_i + g_c - g_q at the cavity of the interval (NaN where it is improper)."""
        data = self._data(input_data) if on_device(self) else None
        if self._native(data):
            e = torch.empty(self.inducing_inputs.shape[0] + 1, dtype=torch.float64, device=self.inducing_inputs.device)
            self._launch(data, input_data[1], 0.0, None, e, None)
            return e
        return self._torch_update(input_data, 0.0)[3]

    def update_sites(self, input_data):
        """One damped PEP update of every site: X_m <- (1 - lr) X_m + lr ((1 - alpha) X_m + sum_{i in m} dX_i) for X = (nat1, nat2,
        log_norm) (sparse_pep.py:473-487)."""
        data = self._data(input_data) if on_device(self) else None
        if self._native(data):
            self._launch(data, input_data[1], self.learning_rate, self.log_norm, None, self.skipped)
            wrote(self.log_norm)
            self._sites_written()
            return
        n1, n2, ln, _, sk = self._torch_update(input_data, self.learning_rate)
        self.nat1, self.nat2 = n1, n2
        self.log_norm = ln[:, None]
        self.skipped = self.skipped + sk.to(self.skipped.device)

    # ---- objectives -----------------------------------------------------------------------------------------------------------------
    def _dist_p_normalizer(self):
        if self._norm_p is None:                     # the prior is fixed
            if on_device(self):
                self._norm_p = self.dist_p.normalizer().reshape(())
            else:
                p = dense_prior(self)
                self._norm_p = 0.5 * (p["P"].shape[0] * math.log(2.0 * math.pi) - p["logdet"])
        return self._norm_p

    def _dist_q_normalizer(self):
        """dist_q.normalizer() = 1/2 (dim log 2 pi - log det Lambda_q + mu_q^T Lambda_q mu_q) without building dist_q and without a
        factorisation of its own: the cached marginals hold log|L| = 1/2 log det Lambda_q and mu_q, and Lambda_q mu_q is the posterior's
        linear natural parameter, the prior's plus the overlap-added nat1 (the packed sites are not unpacked)."""
        if not on_device(self):
            P, mu, _ = dense_posterior(self)
            return 0.5 * (P.shape[0] * math.log(2.0 * math.pi) - torch.linalg.slogdet(P)[1] + mu @ P @ mu)
        p = self.dist_p
        d = p.d
        m, pn = self._marginals(), self._prior_natural()
        quad = (m["mu"] * (pn["lin"] + self._nat1[1:, :d] + self._nat1[:-1, d:])).sum()
        return 0.5 * float(p.T * d) * math.log(2.0 * math.pi) - m["logdetL"].reshape(()) + 0.5 * quad

    def elbo_and_grad(self, input_data):
        raise NotImplementedError("elbo_and_grad is not implemented for SparsePowerExpectationPropagation: its objective is the "
                                  "energy, not the ELBO that SparseCVIGaussianProcess.elbo_and_grad differentiates")

    def energy(self, input_data):
        """The PEP energy  dist_q.normalizer() - dist_p.normalizer() + 1/alpha sum_m sum_{i in m} e_i  (sparse_pep.py:489-495, e_i at the
        cavity); a scalar tensor.  At the fixed point of a Gaussian likelihood with at most one point per interval it is
        log N(y; 0, W K_uu W^T + diag(alpha c + s^2)) - (1 - alpha) / (2 alpha) sum_i log(1 + alpha c_i / s^2)."""
        return self._dist_q_normalizer() - self._dist_p_normalizer() + self.compute_log_norm(input_data).sum() / self.alpha

    def classic_elbo(self, input_data):
        """sum_i E_q log p(y_i | f_i) - KL[q(u) || p(u)] (sparse_pep.py:520-542), with the wrapped likelihood's variational
        expectations."""
        if on_device(self):
            return super().classic_elbo(input_data)
        idx, w, c, y = self._torch_terms(input_data)
        mu, S = self.compute_marginals()
        fmu = (w * mu[idx]).sum(-1)
        fvar = torch.einsum("pi,pij,pj->p", w, S[idx], w) + c
        ve = self._likelihood.variational_expectations(fmu[:, None], fvar[:, None], y[:, None]).sum()
        P, mq, Sq = dense_posterior(self)
        p = dense_prior(self)
        kl = 0.5 * ((p["P"] * Sq).sum() + mq @ p["P"] @ mq - P.shape[0] - p["logdet"] - torch.linalg.slogdet(Sq)[1])
        return ve - kl

    def elbo(self, input_data):
        return self.classic_elbo(input_data)

    def loss(self, input_data):
        return -self.elbo(input_data)

    @property
    def posterior(self):
        if not on_device(self):
            raise NotImplementedError("the posterior process needs the sites on the device")
        return super().posterior
