"""
Sparse CVI with several latent processes under one coupled likelihood: `MultiLatentSparseCVI` fits the reference's
MultiStageLikelihood (markovflow/likelihoods/mutlistage_likelihood.py, three latents) and the two-latent heteroskedastic Gaussian of its
docs/notebooks/stacked_kernels.py with sites on pairs of consecutive inducing states (the reference runs both under SVGP; this project's
inducing-state model is sparse CVI, DESIGN.md sections 8 and 20).

The latents are independent a priori (IndependentMultiOutput: one state of D = sum dl, latent l in the slots off_l .. off_l + dl[l]) and
the likelihoods take the factorised marginals q(F) = prod_l q(F_l), so the projection of a data point onto latent l touches latent l's
slots of the pair only, the site of an interval is block-diagonal over latents, and one row h_i [2D] = sum_l (H P_i)[l, :] carries all
L projections.

Routes.  Device (sorted, un-batched time points on the GPU): per step one factorisation and one selected inverse (the parent's
_marginals), one mfgm_ml_predict_lik (marginals of every latent, the likelihood, its gradients, the per-interval VE sums) and one
mfgm_ml_site_update[_q]; the predict-lik result is cached on the sites' Stamp, so `update_sites; classic_elbo` costs one of each.
Torch (VIDP_NATIVE_ML=0, CPU tensors or unsorted times): materialised rows W [N, L, 2D], the pair marginals, the likelihood classes'
torch formulas and index_add_; on CPU tensors a dense posterior over all inducing states (small models, the host tests;
pair_sites.py).  The data cache, the site-update dispatch, the graph capture, the pair marginals and the KL term are
DenseRouteSparseCVI's (sparse_variational_cvi.py).
"""
import ctypes
import os

import torch

from . import _lib
from .conditionals import _cond_stats
from .kernels import IndependentMultiOutput, PiecewiseKernel
from .packed import _ptr, _stream
from .pair_sites import csr_offsets, initial_state, slot_mask
from .sparse_variational_cvi import DenseRouteSparseCVI
from .stamps import Stamp

MAX_STATE_DIM = 32


class MultiLatentSparseCVI(DenseRouteSparseCVI):
    """kernel: an IndependentMultiOutput whose output_dim equals likelihood.latent_dim (time-invariant emission, state_dim <= 32);
    inducing_points [M] (sorted, one chain); likelihood: MultiStageLikelihood or HeteroskedasticGaussian (vidp_amd.likelihoods).
    Data: (time_points [N], observations [N, 1])."""

    PREDICT_CHUNK = 16384          # points whose [2D, 2D] pair covariances the torch route gathers at a time

    def __init__(self, kernel, inducing_points, likelihood, mean_function=None, learning_rate=0.1, shard=None):
        if mean_function is not None:
            raise NotImplementedError("MultiLatentSparseCVI does not take a mean function (mean_function=)")
        if shard is not None:
            raise NotImplementedError("MultiLatentSparseCVI does not share its chain between processes (shard=)")
        if not isinstance(kernel, IndependentMultiOutput):
            raise TypeError("kernel must be an IndependentMultiOutput: one child kernel per latent of the likelihood")
        if any(isinstance(k, PiecewiseKernel) for k in kernel.kernels):
            raise NotImplementedError("MultiLatentSparseCVI does not take PiecewiseKernel children: the stacked state is a Sum of "
                                      "stationary kernels")
        L = getattr(likelihood, "latent_dim", None)
        if L is None or kernel.output_dim != L:
            raise ValueError(f"the kernel has {kernel.output_dim} outputs and the likelihood {L} latents: they must agree")
        if inducing_points.dim() != 1:
            raise NotImplementedError("one chain: inducing_points [M]; batched inducing points are not supported")
        if kernel.state_dim > MAX_STATE_DIM or kernel.state_dim < 2:
            raise ValueError(f"state dimension {kernel.state_dim} is outside 2 .. {MAX_STATE_DIM}")
        H = kernel.generate_emission_model(inducing_points[:1]).constant_matrix
        if H is None:
            raise NotImplementedError("the kernel's emission matrix must be time-invariant")
        super().__init__(kernel, inducing_points, likelihood, None, learning_rate)
        self._dl = [int(k.state_dim) for k in kernel.kernels]
        self._emission = H.to(inducing_points.device, torch.float64)          # [L, D]
        self._slot_mask = slot_mask(self._dl, inducing_points.device)       # [L, 2D]: the slots of the pair that latent l owns

    @property
    def latent_dim(self):
        return self._likelihood.latent_dim

    # ---- per-data-set constants ----------------------------------------------------------------------------------------------------------
    def _features(self, t):
        """W [N, L, 2D] (row l supported on latent l's slots), c [N, L], interval index [N] of the time points t [N]."""
        if t.dim() != 1:
            raise NotImplementedError("time points are [N]; batched time points are not supported")
        P, Tc, idx = _cond_stats(t.contiguous(), self.inducing_inputs, self._kernel)
        H = self._emission
        W = torch.einsum("lk,nkj->nlj", H, P) * self._slot_mask
        c = torch.einsum("lk,nkj,lj->nl", H, Tc, H)
        return W, c.contiguous(), idx

    def projection_inducing_states_to_observations(self, input_data):
        """[N, L, 2D]: the projection of F(t_i) onto the pair of inducing states around t_i."""
        t = input_data[0] if isinstance(input_data, (tuple, list)) else input_data
        return self._features(t)[0]

    def _build_data(self, t):
        """Constants of the device route (sorted times on the GPU): CSR offsets, h [N, 2D], c [N, L], the prior's initial state; None
        where the torch route applies."""
        z = self.inducing_inputs
        if not (t.dim() == 1 and t.is_cuda and z.is_cuda and os.environ.get("VIDP_NATIVE_ML", "1") != "0"
                and (t.numel() < 2 or bool((t[1:] >= t[:-1]).all()))):
            return None
        M, D, L, N = int(z.shape[0]), self._kernel.state_dim, self.latent_dim, int(t.shape[0])
        if N > 0:
            W, cc, idx = self._features(t)
            h = W.sum(1).contiguous()
        else:
            mk = lambda *s: torch.zeros(s, dtype=torch.float64, device=z.device)
            h, cc, idx = mk(1, 2 * D), mk(1, L), torch.zeros(0, dtype=torch.int64, device=z.device)
        seg = csr_offsets(idx, M + 1)
        pm, pc = initial_state(self._kernel, z)
        sd = _lib.MlData()
        sd.M, sd.L, sd.N = M, L, N
        for l, n in enumerate(self._dl):
            sd.dl[l] = n
        sd.seg, sd.h, sd.c, sd.prior_mean, sd.prior_cov = seg.data_ptr(), h.data_ptr(), cc.data_ptr(), pm.data_ptr(), pc.data_ptr()
        return dict(struct=sd, keep=(seg, h, cc, pm, pc), N=N)

    def _lik_struct(self, kind=None):
        lk = _lib.MlLik()
        lk.kind = self._likelihood.ml_kind if kind is None else kind
        lk.param[0], lk.param[1] = self._likelihood.ml_params
        return lk

    # ---- device route ------------------------------------------------------------------------------------------------------------------
    def _predict_lik(self, data, Y):
        """dict(fmu, fvar, g1, g2 [N, L], ve_part [M + 1]) at the data points for the current sites: one launch (mfgm_ml_predict_lik),
        cached until the sites, the data set or the observations move."""
        c = getattr(self, "_ml_cache", None)
        if c is not None and self._current(c[0]) and c[1] is data and c[2].matches(Y):
            return c[3]
        if Y.shape != (data["N"], 1) or Y.dtype != torch.float64 or not Y.is_cuda:
            raise ValueError("observations must be a float64 [N, 1] tensor on the model's device")
        y = Y.contiguous()
        m = self._marginals()
        pl, N, L = self.dist_p.plan, data["N"], self.latent_dim
        out = torch.empty((4, max(N, 1), L), dtype=torch.float64, device=pl.device)[:, :N]
        ve = torch.empty(self.inducing_inputs.shape[0] + 1, dtype=torch.float64, device=pl.device)
        lk = self._lik_struct()
        _lib.check(pl.lib.mfgm_ml_predict_lik(ctypes.byref(data["struct"]), ctypes.byref(lk), _ptr(y), _ptr(m["mu"]), _ptr(m["Sig"]),
                                              _ptr(m["Sub"]), _ptr(out[0]), _ptr(out[1]), _ptr(ve), _ptr(out[2]), _ptr(out[3]), _stream()),
                   "mfgm_ml_predict_lik")
        res = dict(fmu=out[0], fvar=out[1], g1=out[2], g2=out[3], ve_part=ve, y=y)
        self._ml_cache = (self._key(), data, Stamp(Y), res)
        return res

    _SITE_UPDATE = ("g1", "g2", "mfgm_ml_site_update", "mfgm_ml_site_update_q")      # gradients of _predict_lik; dense, packed entry

    def update_sites(self, input_data):
        """theta_m <- (1 - rho) theta_m + rho sum_{i in m} (g1_i, g2_i projected through h_i), block-diagonal over latents."""
        data = self._data(input_data)
        if data is None:
            return self._update_sites_torch(input_data)
        r = self._predict_lik(data, input_data[1])
        g1, g2, dense, packed = self._SITE_UPDATE
        self._site_update(data, r[g1], r[g2], float(self.learning_rate), dense, packed)

    def step_graph(self, input_data):
        """`update_sites(input_data); classic_elbo(input_data)` captured once in a HIP graph (device route): returns a callable that
        replays it and hands back the ELBO, a device scalar that every replay overwrites."""
        return self._step_graph(input_data, "_ml_cache")

    # ---- torch route (the correctness anchor) ----------------------------------------------------------------------------------------------
    def _predict_torch(self, t):
        """(fmu, fvar [N, L], W [N, L, 2D], interval index) at any time points, sorted or not."""
        W, c, idx = self._features(t)
        pm, pc = self._pair_marginals()
        fmu = torch.einsum("nlj,nj->nl", W, pm[idx])
        fvar = c.clone()
        for lo in range(0, W.shape[0], self.PREDICT_CHUNK):          # the pair covariances are gathered a chunk of points at a time
            sl = slice(lo, lo + self.PREDICT_CHUNK)
            fvar[sl] += torch.einsum("nli,nij,nlj->nl", W[sl], pc[idx[sl]], W[sl])
        return fmu, fvar, W, idx

    def _update_sites_torch(self, input_data):
        t, Y = input_data
        fmu, fvar, W, idx = self._predict_torch(t)
        g1, g2 = self._likelihood.ve_gradients_expectation(fmu, fvar, Y)
        s1 = torch.zeros_like(self.nat1).index_add_(0, idx, torch.einsum("nl,nlj->nj", g1, W))
        s2 = torch.zeros_like(self.nat2)
        for lo in range(0, W.shape[0], self.PREDICT_CHUNK):
            sl = slice(lo, lo + self.PREDICT_CHUNK)
            s2.index_add_(0, idx[sl], torch.einsum("nl,nli,nlj->nij", g2[sl], W[sl], W[sl]))
        lr = self.learning_rate
        self.nat1 = (1 - lr) * self.nat1 + lr * s1      # (the setters move the stamps)
        self.nat2 = (1 - lr) * self.nat2 + lr * s2

    # ---- public interface ------------------------------------------------------------------------------------------------------------------
    def predict_f(self, time_points):
        """Marginal (means, variances) [N, L] of the L latents at any time points."""
        data = self._data((time_points,), keep=False)
        if data is None:
            fmu, fvar, _, _ = self._predict_torch(time_points)
            return fmu, fvar
        m = self._marginals()
        pl, N, L = self.dist_p.plan, data["N"], self.latent_dim
        out = torch.empty((2, max(N, 1), L), dtype=torch.float64, device=pl.device)[:, :N]
        lk = self._lik_struct(_lib.ML_NONE)
        _lib.check(pl.lib.mfgm_ml_predict_lik(ctypes.byref(data["struct"]), ctypes.byref(lk), None, _ptr(m["mu"]), _ptr(m["Sig"]),
                                              _ptr(m["Sub"]), _ptr(out[0]), _ptr(out[1]), None, None, None, _stream()),
                   "mfgm_ml_predict_lik")
        return out[0], out[1]

    def predict_f_at_data(self, input_data):
        """Marginal (means, variances) [N, L] at the data points (from the cached predict-lik pass on the device route)."""
        data = self._data(input_data)
        if data is None:
            return self.predict_f(input_data[0])
        r = self._predict_lik(data, input_data[1])
        return r["fmu"], r["fvar"]

    def local_objective_and_gradients(self, Fmu, Fvar, Y):
        """(sum of variational expectations, (g1, g2) [N, L] with respect to the expectation parameters of every latent)."""
        return (self._likelihood.variational_expectations(Fmu, Fvar, Y).sum(), self._likelihood.ve_gradients_expectation(Fmu, Fvar, Y))

    def elbo_and_grad(self, input_data):
        raise NotImplementedError("elbo_and_grad is not implemented for MultiLatentSparseCVI: IndependentMultiOutput is outside the "
                                  "kernel score (DESIGN.md section 21)")

    def classic_elbo(self, input_data):
        """sum_i E_q log p(y_i | F_i) - KL[q(s_Z) || p(s_Z)]."""
        data = self._data(input_data)
        if data is None:
            fmu, fvar = self.predict_f(input_data[0])
            return self._likelihood.variational_expectations(fmu, fvar, input_data[1]).sum() - self._kl()
        return self._predict_lik(data, input_data[1])["ve_part"].sum() - self._kl()

    elbo = classic_elbo

    def predict_log_density(self, input_data, full_output_cov=False):
        """Forwards to the likelihood (which raises for both multi-latent likelihoods, as in the reference)."""
        t, Y = input_data
        return self._likelihood.predict_log_density(*self.predict_f(t), Y)
