"""
Host-side mirror of markovflow/models/spatio_temporal_variational.py `SpatioTemporalSparseCVI` (:360-586): sparse CVI on pairs of
inducing states for k((x, t), (x', t')) = k_s(x, x') k_t(t, t'), the state being Ms independent copies of the time kernel's (one per
spatial inducing point, D = Ms d_t).  It is SparseCVIGaussianProcess with a Kronecker-factored projection

    w_i[half D + j d_t + k] = a_i[j] h_i[half d_t + k],   a_i = chol(K_zz)^-1 k_s(Z_s, x_i),   h_i = H_t P^t_i

and the conditional variance  c_i = k_s(x_i, x_i) - |a_i|^2 + |a_i|^2 H_t T^t_i H_t^T  (space_time_predict_f ->
batch_base_conditional, :149-183; K_nn - Q_nn is not scaled by the time kernel's variance, as in the reference).  The marginals, the
packed sites, the inverse / Cholesky form choice, the KL-terms cache and the one-launch ELBO are SparseCVIGaussianProcess's; the data
cache, the site-update dispatch, the pair marginals and the KL term of both devices are DenseRouteSparseCVI's.

Routes: CPU tensors, unsorted times or VIDP_FUSED_SPARSE=0 take the torch route (searchsorted + index_add; w formed from a and h by
broadcasting; conditional_statistics runs on the time kernel only, no [N, D, 2D] tensor); on the device with sorted times D <= 8
materialises w [N, 2D] for mfgm_sparse_predict / mfgm_sparse_site_update, 8 < D <= 32 runs mfgm_st_predict_kl /
mfgm_st_site_update_q on (a, h) and never forms w (VIDP_ST_FACTORED=0: the materialised w through mfgm_sparse_predict_kl /
mfgm_sparse_site_update_q instead, the yardstick of tools/st_rate.py).
"""
import ctypes
import os

import torch

from . import _lib
from .conditionals import _cond_stats
from .kernels import PiecewiseKernel, SparseSpatioTemporalKernel
from .packed import _ptr, _stream
from .pair_sites import csr_offsets, initial_state
from .sparse_variational_cvi import DenseRouteSparseCVI

MAX_STATE_DIM = 32


class SpatioTemporalSparseCVI(DenseRouteSparseCVI):
    """inducing_space [Ms, p], inducing_time [M_t] (sorted), kernel_space (vidp_amd.space_kernels), kernel_time (vidp_amd.kernels),
    likelihood (Gaussian, Bernoulli, Poisson, ScalarQuadratureLikelihood), mean_function: any callable X [N, p + 1] -> [N, 1].
    Data: X [N, p + 1] with time in the last column, Y [N, 1]."""

    PREDICT_CHUNK = 16384          # points whose [2D, 2D] pair covariances the torch route gathers at a time (at most 0.5 GB)

    def __init__(self, inducing_space, inducing_time, kernel_space, kernel_time, likelihood, mean_function=None, learning_rate=0.1,
                 num_data=None, shard=None):
        if shard is not None:
            raise NotImplementedError("SpatioTemporalSparseCVI does not share its chain between processes (shard=)")
        if num_data is not None:
            raise NotImplementedError("minibatch scaling (num_data=) is not supported")
        if inducing_time.dim() != 1 or torch.as_tensor(inducing_space).dim() != 2:
            raise NotImplementedError("one chain: inducing_time [M_t] and inducing_space [Ms, p]; batched inducing points are not supported")
        if mean_function is not None and not callable(mean_function):
            raise ValueError("mean_function must be a callable X -> [N, 1]")
        if isinstance(kernel_time, PiecewiseKernel):
            raise NotImplementedError("SpatioTemporalSparseCVI does not take a PiecewiseKernel as its time kernel: the stacked state is a "
                                      "Sum of stationary kernels")
        inducing_space = torch.as_tensor(inducing_space, dtype=torch.float64).to(inducing_time.device)
        Ms, d_t = int(inducing_space.shape[0]), int(kernel_time.state_dim)
        if Ms * d_t > MAX_STATE_DIM:
            raise ValueError(f"state dimension Ms * d_t = {Ms} * {d_t} = {Ms * d_t} exceeds the limit of {MAX_STATE_DIM}")
        kernel = SparseSpatioTemporalKernel(kernel_space, kernel_time, inducing_space)
        kernel._time_emission_row(inducing_time.device)          # raises for an emission that depends on time
        super().__init__(kernel, inducing_time, likelihood, None, learning_rate)       # (the mean here is a function of X, applied below)
        self._kernel_space, self._kernel_time = kernel_space, kernel_time
        self._inducing_space, self._mean_function = inducing_space, mean_function
        self.num_inducing_space, self.num_inducing_time = Ms, int(inducing_time.shape[0])

    @property
    def inducing_time(self):
        return self.inducing_inputs

    @property
    def inducing_space(self):
        return self._inducing_space

    # ---- per-data-set constants ----------------------------------------------------------------------------------------------------------
    def _features(self, X):
        """a [N, Ms], h [N, 2 d_t], c [N], interval index [N] of the points X [N, p + 1] (functions of the inputs and the kernels only)."""
        if X.dim() != 2 or X.shape[-1] < 2:
            raise ValueError("inputs are [N, p + 1] with time in the last column")
        x, t = X[:, :-1], X[:, -1].contiguous()
        a, resid = self._kernel.spatial_features(x)
        P, Tc, idx = _cond_stats(t, self.inducing_inputs, self._kernel_time)      # the time kernel alone: [N, d_t, 2 d_t]
        Ht = self._kernel._time_emission_row(X.device)
        h = torch.einsum("k,nkl->nl", Ht, P).contiguous()
        ct = torch.einsum("k,nkl,l->n", Ht, Tc, Ht)
        return a, h, (resid + (a * a).sum(-1) * ct).contiguous(), idx

    @staticmethod
    def _kron_w(a, h):
        """w [N, 2D] from a [N, Ms] and h [N, 2 d_t]."""
        N, Ms = a.shape
        d_t = h.shape[1] // 2
        return (a[:, None, :, None] * h.view(N, 2, 1, d_t)).reshape(N, 2 * Ms * d_t)

    def projection_inducing_states_to_observations(self, input_data):
        """[N, 1, 2D]: the projection of f(x_i, t_i) onto the pair of inducing states around t_i (:494-507)."""
        X = input_data[0] if isinstance(input_data, (tuple, list)) else input_data
        a, h, _, _ = self._features(X)
        return self._kron_w(a, h)[:, None, :]

    def _mean(self, X):
        if self._mean_function is None:
            return None
        m = self._mean_function(X)
        if tuple(m.shape) != (X.shape[0], 1):
            raise ValueError("mean_function must return [N, 1]")
        return m.to(torch.float64)

    def _build_data(self, X):
        """Constants of the device routes (sorted times): CSR offsets, (a, h, c) or the materialised w, the mean function at the data;
        None where the torch route applies."""
        val = None
        z = self.inducing_inputs
        if (X.dim() == 2 and X.is_cuda and z.is_cuda and os.environ.get("VIDP_FUSED_SPARSE", "1") != "0"
                and (X.shape[0] < 2 or bool((X[1:, -1] >= X[:-1, -1]).all()))):
            M, D, N = int(z.shape[0]), self._kernel.state_dim, int(X.shape[0])
            Ms, d_t = self.num_inducing_space, self._kernel_time.state_dim
            if N > 0:
                a, h, cc, idx = self._features(X)
            else:
                mk = lambda *s: torch.zeros(s, dtype=torch.float64, device=z.device)
                a, h, cc, idx = mk(1, Ms), mk(1, 2 * d_t), mk(1), torch.zeros(0, dtype=torch.int64, device=z.device)
            seg = csr_offsets(idx, M + 1)
            pm, pc = initial_state(self._kernel, z)
            factored = D > 8 and self._packed and os.environ.get("VIDP_ST_FACTORED", "1") != "0"
            if factored:
                sd = _lib.StData()
                sd.M, sd.Ms, sd.dt, sd.N = M, Ms, d_t, N
                sd.seg, sd.a, sd.h, sd.c = seg.data_ptr(), a.data_ptr(), h.data_ptr(), cc.data_ptr()
                keep = (seg, a, h, cc, pm, pc)
            else:
                w = self._kron_w(a, h).contiguous()
                sd = _lib.SparseData()
                sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = M, D, N, 0, M + 1
                sd.seg, sd.w, sd.c = seg.data_ptr(), w.data_ptr(), cc.data_ptr()
                keep = (seg, w, cc, pm, pc)
            sd.prior_mean, sd.prior_cov = pm.data_ptr(), pc.data_ptr()
            val = dict(struct=sd, keep=keep, N=N, own=slice(None), factored=factored, mean=self._mean(X))
        return val

    # ---- device routes ---------------------------------------------------------------------------------------------------------------
    def _predict_f_data(self, data):
        """(fmu, fvar) [N, 1] at the data points from the cached marginals, the mean function included."""
        c = getattr(self, "_pred_cache", None)
        if c is not None and self._current(c[0]) and c[1] is data:
            return c[2]
        res = self._predict_compute(data)
        self._pred_cache = (self._key(), data, res)
        return res

    def _predict_compute(self, data):
        if not data["factored"]:
            fmu, fvar = super()._predict_f_data(data)          # (it leaves a cache entry without the mean function: the callers overwrite it)
        else:
            m = self._marginals()
            pl, pn, N = self.dist_p.plan, self._prior_natural(), data["N"]
            out = torch.empty((2, max(N, 1)), dtype=torch.float64, device=pl.device)[:, :N]
            kt = torch.empty(2, dtype=torch.float64, device=pl.device)
            _lib.check(pl.lib.mfgm_st_predict_kl(ctypes.byref(data["struct"]), _ptr(m["mu"]), _ptr(m["Sig"]), _ptr(m["Sub"]), _ptr(out[0]),
                                                 _ptr(out[1]), pl.h, _ptr(pn["nat"]["diag"]), _ptr(pn["nat"]["sub"]), -2.0, -1.0,
                                                 _ptr(self._prior_mean_packed()), _ptr(kt[0:1]), _ptr(kt[1:2]), _ptr(pl.ws), _stream()),
                       "mfgm_st_predict_kl")
            self._kl_cache = (self._key(), kt[0:1], kt[1:2])
            fmu, fvar = out[0][:, None], out[1][:, None]
        if data["mean"] is not None:
            fmu = fmu + data["mean"]
        return fmu, fvar

    def _gradients(self, fmu, fvar, Y, mean):
        """Likelihood gradients with respect to the expectation parameters of the CENTRED f (:571-574): evaluated at F = F_c + m,
        g1 = g1' + 2 g2 m, g2 = g2'."""
        g1, g2 = self._likelihood.ve_gradients_expectation(fmu, fvar, Y)
        if mean is not None:
            g1 = g1 + 2.0 * g2 * mean
        return g1, g2

    def local_objective_and_gradients(self, Fmu, Fvar, X, Y):
        """(sum of variational expectations, gradients with respect to [mu, sigma^2 + mu^2] of the centred f) (:554-576)."""
        obj = self._likelihood.variational_expectations(Fmu, Fvar, Y).sum()
        return obj, self._gradients(Fmu, Fvar, Y, self._mean(X))

    def update_sites(self, input_data):
        """theta_m <- (1 - rho) theta_m + rho g_m (:509-552)."""
        data = self._data(input_data)
        if data is None:
            return self._update_sites_torch(input_data)
        _, Y = input_data
        fmu, fvar = self._predict_f_data(data)
        g1, g2 = self._gradients(fmu, fvar, Y, data["mean"])
        g1, g2 = g1.reshape(-1).contiguous(), g2.reshape(-1).contiguous()
        self._site_update(data, g1, g2, float(self.learning_rate), "mfgm_sparse_site_update",
                          "mfgm_st_site_update_q" if data["factored"] else "mfgm_sparse_site_update_q")

    # ---- torch route (the correctness anchor) ----------------------------------------------------------------------------------------------
    def _predict_torch(self, X):
        """(fmu, fvar [N, 1] with the mean function, w [N, 2D], interval index) at any inputs, sorted or not."""
        a, h, c, idx = self._features(X)
        w = self._kron_w(a, h)
        pm, pc = self._pair_marginals()
        fmu = (w * pm[idx]).sum(-1)
        fvar = c.clone()
        for lo in range(0, w.shape[0], self.PREDICT_CHUNK):          # the pair covariances are gathered a chunk of points at a time
            sl = slice(lo, lo + self.PREDICT_CHUNK)
            fvar[sl] += torch.einsum("ni,nij,nj->n", w[sl], pc[idx[sl]], w[sl])
        mean = self._mean(X)
        fmu = fmu[:, None] if mean is None else fmu[:, None] + mean
        return fmu, fvar[:, None], w, idx, mean

    def space_time_predict_f(self, inputs):
        """Marginal (mean, variance) [N, 1] of f at inputs [N, p + 1] (:149-183)."""
        data = self._data((inputs,), keep=False)
        if data is not None:                                         # sorted inputs on the device: the kernels of update_sites
            kept = getattr(self, "_data_cache", None)
            if kept is not None and data is kept[1]:                 # the training inputs: their predictions are cached too
                return self._predict_f_data(data)
            keep = getattr(self, "_pred_cache", None)
            res = self._predict_compute(data)
            self._pred_cache = keep
            return res
        fmu, fvar, _, _, _ = self._predict_torch(inputs)
        return fmu, fvar

    def _update_sites_torch(self, input_data):
        X, Y = input_data
        fmu, fvar, w, idx, mean = self._predict_torch(X)
        g1, g2 = self._gradients(fmu, fvar, Y, mean)
        s1 = torch.zeros_like(self.nat1).index_add_(0, idx, g1 * w)
        s2 = torch.zeros_like(self.nat2).index_add_(0, idx, g2[:, :, None] * w[:, :, None] * w[:, None, :])
        lr = self.learning_rate
        self.nat1 = (1 - lr) * self.nat1 + lr * s1      # (the setters move the stamps)
        self.nat2 = (1 - lr) * self.nat2 + lr * s2

    def elbo_and_grad(self, input_data):
        raise NotImplementedError("elbo_and_grad is not implemented for SpatioTemporalSparseCVI: the spatial kernel and the Kronecker "
                                  "state are outside the kernel score (DESIGN.md section 21)")

    def classic_elbo(self, input_data):
        """sum_i E_q log p(y_i | f_i) - KL[q(s(Z_t)) || p(s(Z_t))] (:209-236)."""
        if self._data(input_data) is not None:
            return super().classic_elbo(input_data)
        X, Y = input_data
        fmu, fvar = self.space_time_predict_f(X)
        return self._likelihood.variational_expectations(fmu, fvar, Y).sum() - self._kl()

    elbo = classic_elbo

    def predict_log_density(self, input_data, full_output_cov=False):
        """log p(y* | data) per point: the likelihood's predict_log_density of space_time_predict_f (:238-246)."""
        X, Y = input_data
        return self._likelihood.predict_log_density(*self.space_time_predict_f(X), Y)
