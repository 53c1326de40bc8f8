"""
Gaussian-process factor analysis by sparse CVI: `FactorAnalysisSparseCVI` fits P observed channels that are linear mixtures
f_p(t) = sum_l W_pl(t) g_l(t), W = A(t) B, of L independent latent GPs (the reference's FactorAnalysisKernel, markovflow/kernels/
sde_kernel.py:881, docs/notebooks/factor_analysis.py -- the GPFA model) with sites on pairs of consecutive inducing states and one
scalar likelihood per output.

The latents are independent a priori (the state of IndependentMultiOutput: D = sum dl, latent l in the slots off_l .. off_l + dl[l]), so
one row h_i [2D] carries the projections of a point onto all L latents, as in the multi-latent model.  The mixing couples them a
posteriori: the marginal of an output needs the cross-latent blocks of the pair covariance and the site of an interval is dense across
latents.  Both enter through L x L matrices only -- the latent marginal (a_i [L], K_i [L, L]) of a point and the mixed gradients
(gam1_i [L], gam2_i [L, L]) -- which is what the device route computes: (2D)^2 + P L^2 multiply-adds per point where P materialised
rows w_ip [2D] cost P (2D)^2.

Routes.  Device (sorted, un-batched time points on the GPU, P <= 64, Gaussian / Bernoulli / Poisson outputs; VIDP_NATIVE_FA=0 disables
it): per step the parent's _marginals() (one factorisation, one selected inverse), one mfgm_fa_predict_lik cached on the sites' Stamp
and one mfgm_fa_site_update[_q], so `update_sites; classic_elbo` costs one of each.  Torch (otherwise): materialised rows
w_ip = sum_l W_ipl (h_i masked to latent l), the pair marginals, the likelihood classes' torch formulas and index_add_, a chunk of
points at a time; on CPU tensors a dense posterior over all inducing states (small models, the host tests; pair_sites.py).  The data
cache, the site-update dispatch, the graph capture, the pair marginals and the KL term are DenseRouteSparseCVI's
(sparse_variational_cvi.py).
"""
import ctypes
import math
import os

import torch

from . import _lib
from .conditionals import _cond_stats
from .kernels import FactorAnalysisKernel
from .likelihoods import Bernoulli, Gaussian, Poisson
from .packed import _ptr, _stream
from .pair_sites import csr_offsets, initial_state, slot_mask
from .sparse_variational_cvi import DenseRouteSparseCVI
from .stamps import Stamp

MAX_STATE_DIM = 32
MAX_NATIVE_OUTPUTS = 64
_KINDS = {Gaussian: _lib.LIK_GAUSSIAN, Bernoulli: _lib.LIK_BERNOULLI, Poisson: _lib.LIK_POISSON}


def _tri_to_full(tri, L):
    """[N, L (L + 1) / 2] lower triangles, row-major -> symmetric [N, L, L]."""
    i, j = torch.tril_indices(L, L, device=tri.device)
    full = torch.zeros((tri.shape[0], L, L), dtype=tri.dtype, device=tri.device)
    full[:, i, j] = tri
    full[:, j, i] = tri
    return full


class FactorAnalysisSparseCVI(DenseRouteSparseCVI):
    """kernel: a FactorAnalysisKernel (state_dim 2 .. 32); inducing_points [M] (sorted, one chain); likelihood: one Gaussian / Bernoulli /
    Poisson / ScalarQuadratureLikelihood for all outputs or a list of P of them.  Data: (time_points [N], observations [N, P]); a NaN
    observation marks a channel not observed at that time."""

    PREDICT_CHUNK = 16384          # rows w_ip whose [2D, 2D] pair covariances the torch route gathers at a time

    def __init__(self, kernel, inducing_points, likelihood, mean_function=None, learning_rate=0.1, shard=None):
        if mean_function is not None:
            raise NotImplementedError("FactorAnalysisSparseCVI does not take a mean function (mean_function=)")
        if shard is not None:
            raise NotImplementedError("FactorAnalysisSparseCVI does not share its chain between processes (shard=)")
        if not isinstance(kernel, FactorAnalysisKernel):
            raise TypeError("kernel must be a FactorAnalysisKernel")
        P = kernel.output_dim
        liks = list(likelihood) if isinstance(likelihood, (list, tuple)) else [likelihood] * P
        if len(liks) != P:
            raise ValueError(f"the kernel has {P} outputs and the likelihood list {len(liks)} entries: they must agree")
        if inducing_points.dim() != 1:
            raise NotImplementedError("one chain: inducing_points [M]; batched inducing points are not supported")
        if kernel.state_dim > MAX_STATE_DIM or kernel.state_dim < 2:
            raise ValueError(f"state dimension {kernel.state_dim} is outside 2 .. {MAX_STATE_DIM}")
        super().__init__(kernel, inducing_points, likelihood, None, learning_rate)
        self._liks = liks
        self._dl = [int(k.state_dim) for k in kernel.kernels]
        dev = inducing_points.device
        self._emission = kernel.latent_components._emission_matrix().to(dev, torch.float64)          # H_1 (+) ... (+) H_L  [L, D]
        self._slot_mask = slot_mask(self._dl, dev)                                                  # [L, 2D]
        # columns that share a likelihood object are evaluated in one call
        groups = {}
        for p, lk in enumerate(liks):
            groups.setdefault(id(lk), (lk, []))[1].append(p)
        self._groups = [(lk, torch.tensor(cols, device=dev)) for lk, cols in groups.values()]

    @property
    def latent_dim(self):
        return self._kernel.latent_dim

    @property
    def output_dim(self):
        return self._kernel.output_dim

    def _native_kinds(self):
        """[(kind, param)] per output, or None when an output's likelihood has no native kind."""
        out = []
        for lk in self._liks:
            kind = _KINDS.get(type(lk))
            if kind is None:
                return None
            out.append((kind, lk.variance if kind == _lib.LIK_GAUSSIAN else lk.param))
        return out

    # ---- per-data-set constants ----------------------------------------------------------------------------------------------------------
    def _features(self, t):
        """Hl [N, L, 2D] (row l: the projection of g_l(t_i) onto the pair, supported on latent l's slots), c [N, L], interval [N]."""
        if t.dim() != 1:
            raise NotImplementedError("time points are [N]; batched time points are not supported")
        Pm, Tc, idx = _cond_stats(t.contiguous(), self.inducing_inputs, self._kernel)
        H = self._emission
        Hl = torch.einsum("lk,nkj->nlj", H, Pm) * self._slot_mask
        c = torch.einsum("lk,nkj,lj->nl", H, Tc, H)
        return Hl, c.contiguous(), idx

    def _weights(self, t, loading=None):
        """W(t) = A(t) B: [P, L] (time-invariant) or [N, P, L]; loading: a B to use instead of the kernel's (loading_grad's check)."""
        if loading is None:
            return self._kernel.weights(t)
        return self._kernel.base_weights(t) @ loading

    def projection_inducing_states_to_observations(self, input_data):
        """[N, P, 2D]: the rows w_ip = sum_l W_ipl Hl[i, l] that project f_p(t_i) onto the pair of inducing states around t_i."""
        t = input_data[0] if isinstance(input_data, (tuple, list)) else input_data
        return self._rows(self._weights(t), self._features(t)[0])

    @property
    def _data_extra(self):
        return (self._kernel.loading_version,)          # the constants hold W: kept until the time points or the loading matrix move

    def _build_data(self, t):
        """Constants of the device route (sorted times on the GPU): CSR offsets, h [N, 2D], c [N, L], W, the prior's initial state; None
        where the torch route applies."""
        z = self.inducing_inputs
        if not (t.dim() == 1 and t.is_cuda and z.is_cuda and os.environ.get("VIDP_NATIVE_FA", "1") != "0"
                and self.output_dim <= MAX_NATIVE_OUTPUTS and self._native_kinds() is not None
                and (t.numel() < 2 or bool((t[1:] >= t[:-1]).all()))):
            return None
        M, D, L, P, N = int(z.shape[0]), self._kernel.state_dim, self.latent_dim, self.output_dim, int(t.shape[0])
        if N > 0:
            Hl, cc, idx = self._features(t)
            h = Hl.sum(1).contiguous()
            W = self._weights(t).contiguous()
        else:
            mk = lambda *s: torch.zeros(s, dtype=torch.float64, device=z.device)
            h, cc, idx, W = mk(1, 2 * D), mk(1, L), torch.zeros(0, dtype=torch.int64, device=z.device), mk(P, L)
        seg = csr_offsets(idx, M + 1)
        pm, pc = initial_state(self._kernel, z)
        sd = _lib.FaData()
        sd.M, sd.L, sd.P, sd.N = M, L, P, N
        for l, n in enumerate(self._dl):
            sd.dl[l] = n
        sd.seg, sd.h, sd.c, sd.w = seg.data_ptr(), h.data_ptr(), cc.data_ptr(), W.data_ptr()
        sd.w_stride = 0 if W.dim() == 2 else P * L
        sd.prior_mean, sd.prior_cov = pm.data_ptr(), pc.data_ptr()
        return dict(struct=sd, keep=(seg, h, cc, W, pm, pc), N=N, W=W, t=t)

    def _lik_struct(self, none=False):
        lk = _lib.FaLik()
        if not none:
            for p, (kind, param) in enumerate(self._native_kinds()):
                lk.kind[p], lk.param[p] = kind, param
        return lk

    # ---- device route ------------------------------------------------------------------------------------------------------------------
    def _predict_lik(self, data, Y):
        """dict(fmu, fvar, dm, dv [N, P], lmu, gam1 [N, L], lcov, gam2 [N, LT], ve_part [M + 1]) at the data points for the current
        sites: one launch (mfgm_fa_predict_lik), cached until the sites, the data set or the observations move."""
        c = getattr(self, "_fa_cache", None)
        if c is not None and self._current(c[0]) and c[1] is data and c[2].matches(Y):
            return c[3]
        N, L, P = data["N"], self.latent_dim, self.output_dim
        if tuple(Y.shape) != (N, P) or Y.dtype != torch.float64 or not Y.is_cuda:
            raise ValueError("observations must be a float64 [N, P] tensor on the model's device")
        y = Y.contiguous()
        m = self._marginals()
        pl, LT = self.dist_p.plan, L * (L + 1) // 2
        mk = lambda k, w: torch.empty((k, max(N, 1), w), dtype=torch.float64, device=pl.device)[:, :N]
        op, ol, ot = mk(4, P), mk(2, L), mk(2, LT)
        ve = torch.zeros(self.inducing_inputs.shape[0] + 1, dtype=torch.float64, device=pl.device)
        lk = self._lik_struct()
        _lib.check(pl.lib.mfgm_fa_predict_lik(ctypes.byref(data["struct"]), ctypes.byref(lk), _ptr(y), _ptr(m["mu"]), _ptr(m["Sig"]),
                                              _ptr(m["Sub"]), _ptr(op[0]), _ptr(op[1]), _ptr(ol[0]), _ptr(ot[0]), _ptr(ve), _ptr(op[2]),
                                              _ptr(op[3]), _ptr(ol[1]), _ptr(ot[1]), _stream()), "mfgm_fa_predict_lik")
        res = dict(fmu=op[0], fvar=op[1], dm=op[2], dv=op[3], lmu=ol[0], gam1=ol[1], lcov=ot[0], gam2=ot[1], ve_part=ve, y=y)
        self._fa_cache = (self._key(), data, Stamp(Y), res)
        return res

    def _predict_only(self, data, outputs=True, latents=False):
        """(fmu, fvar, lmu, lcov) (None where not asked for) at the points of `data` for the current sites, no likelihood."""
        m = self._marginals()
        pl, N, L, P = self.dist_p.plan, data["N"], self.latent_dim, self.output_dim
        mk = lambda w: torch.empty((max(N, 1), w), dtype=torch.float64, device=pl.device)[:N]
        fmu, fvar = (mk(P), mk(P)) if outputs else (None, None)
        lmu, lcov = (mk(L), mk(L * (L + 1) // 2)) if latents else (None, None)
        lk = self._lik_struct(none=True)
        _lib.check(pl.lib.mfgm_fa_predict_lik(ctypes.byref(data["struct"]), ctypes.byref(lk), None, _ptr(m["mu"]), _ptr(m["Sig"]),
                                              _ptr(m["Sub"]), _ptr(fmu), _ptr(fvar), _ptr(lmu), _ptr(lcov), None, None, None, None, None,
                                              _stream()), "mfgm_fa_predict_lik")
        return fmu, fvar, lmu, lcov

    _SITE_UPDATE = ("gam1", "gam2", "mfgm_fa_site_update", "mfgm_fa_site_update_q")      # gradients of _predict_lik; dense, packed entry

    def update_sites(self, input_data):
        """theta_m <- (1 - rho) theta_m + rho sum_{i in m} sum_p (g1_ip w_ip, g2_ip w_ip w_ip^T), dense across latents."""
        data = self._data(input_data)
        if data is None:
            return self._update_sites_torch(input_data)
        r = self._predict_lik(data, input_data[1])
        g1, g2, dense, packed = self._SITE_UPDATE
        self._site_update(data, r[g1], r[g2], float(self.learning_rate), dense, packed)

    def step_graph(self, input_data):
        """`update_sites(input_data); classic_elbo(input_data)` captured once in a HIP graph (device route): returns a callable that
        replays it and hands back the ELBO, a device scalar that every replay overwrites (as MultiLatentSparseCVI.step_graph)."""
        return self._step_graph(input_data, "_fa_cache")

    # ---- torch route (the correctness anchor) ----------------------------------------------------------------------------------------------
    def _rows(self, W, Hl):
        """w [n, P, 2D] = sum_l W[n, p, l] Hl[n, l, :]; W [P, L] serves every point."""
        return torch.einsum("pl,nlj->npj" if W.dim() == 2 else "npl,nlj->npj", W, Hl)

    def _predict_torch(self, t, loading=None):
        """(fmu, fvar [N, P], W, Hl [N, L, 2D], c [N, L], interval index) at any time points, sorted or not, from materialised rows."""
        Hl, c, idx = self._features(t)
        W = self._weights(t, loading)
        pm, pc = self._pair_marginals()
        N, P = Hl.shape[0], self.output_dim
        Wn = W if W.dim() == 3 else W.expand(N, *W.shape)
        fmu = torch.einsum("npl,nlj,nj->np", Wn, Hl, pm[idx])
        fvar = torch.einsum("npl,nl->np", Wn * Wn, c)
        step = max(1, self.PREDICT_CHUNK // P)
        parts = []
        for lo in range(0, N, step):          # the pair covariances are gathered a chunk of points at a time
            sl = slice(lo, lo + step)
            w = self._rows(Wn[sl], Hl[sl])
            parts.append(torch.einsum("npi,nij,npj->np", w, pc[idx[sl]], w))
        if parts:
            fvar = fvar + torch.cat(parts, 0)
        return fmu, fvar, Wn, Hl, c, idx

    def _lik_terms(self, fmu, fvar, Y, grads=True):
        """(ve, dm, dv) [N, P] of the outputs' likelihoods (torch formulas; the likelihood classes' own native kernels where they
        apply); a NaN observation gives zeros.  grads=False: ve alone, differentiable in fmu / fvar."""
        seen = ~torch.isnan(Y)
        y0 = torch.where(seen, Y, torch.zeros_like(Y))
        ve, dm, dv = torch.zeros_like(fmu), torch.zeros_like(fmu), torch.zeros_like(fmu)
        for lk, cols in self._groups:
            m, v, yy = (x[:, cols].reshape(-1, 1).contiguous() for x in (fmu, fvar, y0))
            shape = (fmu.shape[0], len(cols))
            e = lk.variational_expectations(m, v, yy)          # Gaussian: element-wise [n, 1]; the quadrature classes: [n]
            ve[:, cols] = e.reshape(shape)
            if grads:
                g1, g2 = lk.ve_gradients_expectation(m, v, yy)
                dv[:, cols] = g2.reshape(shape)
                dm[:, cols] = (g1 + 2.0 * g2 * m).reshape(shape)
        zero = torch.zeros_like(ve)
        return torch.where(seen, ve, zero), torch.where(seen, dm, zero), torch.where(seen, dv, zero)

    def _update_sites_torch(self, input_data):
        t, Y = input_data
        fmu, fvar, Wn, Hl, _, idx = self._predict_torch(t)
        _, dm, dv = self._lik_terms(fmu, fvar, Y)
        g1 = dm - 2.0 * dv * fmu
        s1, s2 = torch.zeros_like(self.nat1), torch.zeros_like(self.nat2)
        step = max(1, self.PREDICT_CHUNK // self.output_dim)
        for lo in range(0, Hl.shape[0], step):
            sl = slice(lo, lo + step)
            w = self._rows(Wn[sl], Hl[sl])
            s1.index_add_(0, idx[sl], torch.einsum("np,npj->nj", g1[sl], w))
            s2.index_add_(0, idx[sl], torch.einsum("np,npi,npj->nij", dv[sl], w, w))
        lr = self.learning_rate
        self.nat1 = (1 - lr) * self.nat1 + lr * s1      # (the setters move the stamps)
        self.nat2 = (1 - lr) * self.nat2 + lr * s2

    def _latents_torch(self, t):
        """(lmu [N, L], K [N, L, L]) at any time points."""
        Hl, c, idx = self._features(t)
        pm, pc = self._pair_marginals()
        lmu = torch.einsum("nlj,nj->nl", Hl, pm[idx])
        K = torch.diag_embed(c)
        step = max(1, self.PREDICT_CHUNK // self.latent_dim)
        parts = []
        for lo in range(0, Hl.shape[0], step):
            sl = slice(lo, lo + step)
            parts.append(torch.einsum("nli,nij,nkj->nlk", Hl[sl], pc[idx[sl]], Hl[sl]))
        if parts:
            K = K + torch.cat(parts, 0)
        return lmu, K

    def ve_sum_torch(self, input_data, loading=None):
        """sum of the variational expectations on the torch route, differentiable in `loading` (a B [L, L] used instead of the
        kernel's): what loading_grad is checked against."""
        t, Y = input_data
        fmu, fvar = self._predict_torch(t, loading)[:2]
        return self._lik_terms(fmu, fvar, Y, grads=False)[0].sum()

    # ---- public interface ------------------------------------------------------------------------------------------------------------------
    def predict_f(self, time_points):
        """Marginal (means, variances) [N, P] of the P outputs at any time points."""
        data = self._data((time_points,), keep=False)
        if data is None:
            fmu, fvar = self._predict_torch(time_points)[:2]
            return fmu, fvar
        if data["N"] == 0:
            z = torch.zeros((0, self.output_dim), dtype=torch.float64, device=time_points.device)
            return z, z.clone()
        return self._predict_only(data)[:2]

    def predict_latents(self, time_points, full_cov=False):
        """Marginal (means [N, L], variances [N, L]) of the L latent GPs at any time points; with full_cov the [N, L, L] covariance
        across latents (the mixing correlates them a posteriori)."""
        data = self._data((time_points,), keep=False)
        L = self.latent_dim
        if data is None:
            lmu, K = self._latents_torch(time_points)
        elif data["N"] == 0:
            lmu = torch.zeros((0, L), dtype=torch.float64, device=time_points.device)
            K = torch.zeros((0, L, L), dtype=torch.float64, device=time_points.device)
        else:
            _, _, lmu, tri = self._predict_only(data, outputs=False, latents=True)
            K = _tri_to_full(tri, L)
        return lmu, (K if full_cov else torch.diagonal(K, dim1=-2, dim2=-1).contiguous())

    def predict_f_at_data(self, input_data):
        """Marginal (means, variances) [N, P] at the data points (from the cached predict-lik pass on the device route)."""
        data = self._data(input_data)
        if data is None or data["N"] == 0:
            return self.predict_f(input_data[0])
        r = self._predict_lik(data, input_data[1])
        return r["fmu"], r["fvar"]

    def local_objective_and_gradients(self, Fmu, Fvar, Y):
        """(sum of variational expectations, (g1, g2) [N, P] with respect to the expectation parameters of every output)."""
        ve, dm, dv = self._lik_terms(Fmu, Fvar, Y)
        return ve.sum(), (dm - 2.0 * dv * Fmu, dv)

    def elbo_and_grad(self, input_data):
        raise NotImplementedError("elbo_and_grad is not implemented for FactorAnalysisSparseCVI: the children's hyper-parameters are "
                                  "outside the kernel score, as for IndependentMultiOutput (DESIGN.md sections 21, 23); loading_grad "
                                  "gives the gradient of the loading matrix")

    def classic_elbo(self, input_data):
        """sum_ip E_q log p(y_ip | f_ip) - KL[q(s_Z) || p(s_Z)]."""
        data = self._data(input_data)
        if data is None:
            fmu, fvar = self.predict_f(input_data[0])
            return self._lik_terms(fmu, fvar, input_data[1], grads=False)[0].sum() - self._kl()
        if data["N"] == 0:
            return -self._kl()
        return self._predict_lik(data, input_data[1])["ve_part"].sum() - self._kl()

    elbo = classic_elbo

    def loading_grad(self, input_data):
        """dELBO/dB [L, L] at fixed sites.  The sites live on the inducing states, so q does not depend on W and the gradient is that of
        the VE term alone: dL/dW_ipl = dm_ip a_il + 2 dv_ip sum_l' W_ipl' K_i[l, l'], dB = sum_i A(t_i)^T dW_i -- torch glue on the latent
        marginals and the likelihood derivatives of the cached predict pass."""
        t, Y = input_data
        data = self._data(input_data)
        L = self.latent_dim
        if data is None or data["N"] == 0:
            fmu, fvar, Wn = self._predict_torch(t)[:3]
            _, dm, dv = self._lik_terms(fmu, fvar, Y)
            lmu, K = self._latents_torch(t)
        else:
            r = self._predict_lik(data, Y)
            dm, dv, lmu, K = r["dm"], r["dv"], r["lmu"], _tri_to_full(r["lcov"], L)
            Wn = data["W"] if data["W"].dim() == 3 else data["W"].expand(data["N"], *data["W"].shape)
        dW = dm[:, :, None] * lmu[:, None, :] + 2.0 * dv[:, :, None] * torch.einsum("npk,nlk->npl", Wn, K)
        A = self._kernel.base_weights(t)
        if A.dim() == 2:
            return A.transpose(0, 1) @ dW.sum(0)
        return torch.einsum("npk,npl->kl", A, dW)

    def predict_log_density(self, input_data, full_output_cov=False):
        """log p(y_i* | data) [N]: the sum over the observed outputs of each likelihood's log predictive density at the output
        marginals (the outputs are taken as independent given their marginals, as the site update takes them)."""
        t, Y = input_data
        fmu, fvar = self.predict_f(t)
        seen = ~torch.isnan(Y)
        y0 = torch.where(seen, Y, torch.zeros_like(Y))
        out = torch.zeros_like(fmu)
        for lk, cols in self._groups:
            m, v, yy = (x[:, cols].reshape(-1, 1) for x in (fmu, fvar, y0))
            if isinstance(lk, Gaussian):
                s = v + lk.variance
                d = (-0.5 * torch.log(2.0 * math.pi * s) - 0.5 * (yy - m) ** 2 / s)[:, 0]
            else:
                d = lk.predict_log_density(m, v, yy)
            out[:, cols] = d.reshape(fmu.shape[0], len(cols))
        return torch.where(seen, out, torch.zeros_like(out)).sum(-1)

    def kernel_changed(self):
        super().kernel_changed()
        self._fa_cache = None
