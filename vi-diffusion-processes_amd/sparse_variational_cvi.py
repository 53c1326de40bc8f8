"""
Host-side mirror of markovflow/models/sparse_variational_cvi.py `SparseCVIGaussianProcess`
(sparse_variational_cvi.py:38-292): CVI with sites on pairs of consecutive inducing states.  The overlap-add of the
[M+1, 2d, 2d] sites into the block-tri-diagonal natural parameters and the data -> site segment sums (a Python list of
M+1 reduce_sums in the reference, :199-213) are single index_add operations; the posterior refresh runs in the HIP sweeps.
`DenseRouteSparseCVI` below it is the parent of the models built on it (sparse_pep.py, spatio_temporal_variational.py,
multi_latent_variational.py, factor_analysis_variational.py): what they share beyond the plain model.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import FULL, SYM, VEC
from .conditionals import _conditional_statistics, conditional_statistics
from .likelihoods import Bernoulli, Gaussian, Poisson
from .packed import Plan, _ptr, _stream
from .pair_sites import chain_kl, csr_offsets, dense_kl, initial_state, need_device, on_device, pair_marginals
from .posterior import ConditionalProcess
from .ssm_gaussian_transformations import naturals_to_ssm_params_packed
from .stamps import Stamp, wrote
from .variational_cvi import back_project_nats

# the likelihoods of the native mini-batch pass (mfgm_sparse_batch_predict_lik): exactly these classes
_BATCH_KINDS = {Gaussian: _lib.LIK_GAUSSIAN, Bernoulli: _lib.LIK_BERNOULLI, Poisson: _lib.LIK_POISSON}


class SparseCVIGaussianProcess:
    """`shard=(rank, world)` (or `(rank, world, allreduce, allgather)` with stand-ins for the collectives, or a dict with these keys and
    optionally the partition `R0`, `Rup`): ONE chain shared between
    `world` processes along time (SURVEY 8e second row, config 5; distributed.ChainShard).  Process k owns the inducing states
    [node_lo, node_hi), the sites / intervals m in [node_lo, node_hi) (interval m lies between states m - 1 and m; the last process also
    takes interval M) and the data points inside them.  Per step three small collectives cross processes: the site on the right edge
    (one [2d + 4d^2] block per neighbour pair, all-gathered after `update_sites`), the exchange level of the factorisation
    (n_X (3d^2 + 2d) doubles) and the four scalars of the ELBO.  Every process is handed the same (time_points, observations) and keeps
    its own slice; the arrays over inducing states keep global indices and are valid on the owned range.  State dimension > 8 only.

    `num_data=N_total` puts the model in MINI-BATCH mode: `update_sites` and `classic_elbo` then take a batch
    (t [n], y [n, 1]) drawn from a data set of N_total points, in any order and a new tensor every step, and weigh its terms by
    num_data / n -- the reference's sparse variational models (models/sparse_variational.py:184-192).  Not with `shard=`."""

    num_data = None          # (a class attribute: the models built on this class do not take the keyword)

    def __init__(self, kernel, inducing_points, likelihood, mean_function=None, learning_rate=0.1, shard=None, num_data=None):
        self._kernel, self._likelihood = kernel, likelihood
        self.learning_rate = learning_rate
        if num_data is not None:
            if shard is not None:
                raise NotImplementedError("mini-batches (num_data=) of a chain shared between processes (shard=) are not implemented")
            if not float(num_data) > 0.0:
                raise ValueError(f"num_data must be positive, got {num_data!r}")
            self.num_data = float(num_data)
        self.inducing_inputs = inducing_points
        M, sd = inducing_points.shape[-1], kernel.state_dim
        dev, dt = inducing_points.device, torch.float64
        self._version = 0          # bumped by every site update: keys the cached posterior marginals
        # Wide path (state dimension > 8): the RESIDENT form of nat2 is the quadrant-packed tensor _nat2q [M + 1, d (d + 1) + d^2]
        # (include/mfgm.h: the lower triangle of each symmetric [2d, 2d] site, 528 instead of 1 024 doubles at d = 16) that the site
        # update and the factor passes work on; `nat2` materialises the reference's [M + 1, 2d, 2d] tensor on demand and takes
        # assignments / in-place edits back (VIDP_PACKED_SITES=0: the dense tensor stays the resident one)
        self._packed = sd > 8 and inducing_points.dim() == 1 and os.environ.get("VIDP_PACKED_SITES", "1") != "0"
        self._nat2q, self._nat2, self._nat2_seen = None, None, None
        self.nat1 = torch.zeros((M + 1, 2 * sd), dtype=dt, device=dev)
        if self._packed:
            self._nat2q = torch.zeros((M + 1, sd * (sd + 1) + sd * sd), dtype=dt, device=dev)
        else:
            self.nat2 = torch.zeros((M + 1, 2 * sd, 2 * sd), dtype=dt, device=dev)
        self._dist_p = None
        self._shard = None
        # a mean function of time (mean_function.py): the sites live on the zero-mean part g, the likelihood sees f = g + m
        self._time_mean = mean_function
        if shard is not None and mean_function is not None:
            raise NotImplementedError("a chain shared between processes (shard=) does not take a mean function")
        if shard is not None:
            from .distributed import ChainShard
            if sd <= 8 or inducing_points.dim() != 1:
                raise ValueError("a chain is shared between processes on the wide path only (state dimension > 8, one chain)")
            if not isinstance(shard, dict):
                shard = dict(zip(("rank", "world", "allreduce", "allgather"), shard))
            rank, world = int(shard["rank"]), int(shard["world"])
            # a plan of its own: the prior's plan keeps serving whole-chain calls (dist_p, dist_q of gathered sites)
            self._shard = ChainShard(Plan(1, M, sd, R0=shard.get("R0", 0), Rup=shard.get("Rup", 0), device=dev), rank, world,
                                     shard.get("allreduce"), shard.get("allgather"))
            self._m_lo = self._shard.node_lo
            self._m_hi = self._shard.node_hi + (1 if rank == world - 1 else 0)

    # the sites are public tensors, as the reference's `sites.nat1 / nat2`: assigning them, or editing them in place through torch, moves
    # the key of every cached posterior quantity (the library's own in-place updates bump `_version`)
    @property
    def nat1(self):
        return self._nat1

    @nat1.setter
    def nat1(self, value):
        self._nat1 = value
        self._version += 1

    def _pack_index(self):
        """Flat indices into a [2d, 2d] site of the entries the packed form keeps, in its order: upper-left lower triangle, lower-left
        block, lower-right lower triangle."""
        idx = getattr(self, "_pidx", None)
        if idx is None:
            d = self._kernel.state_dim
            d2 = 2 * d
            i, j = torch.tril_indices(d, d)
            r, c = torch.meshgrid(torch.arange(d), torch.arange(d), indexing="ij")
            idx = torch.cat([i * d2 + j, ((d + r) * d2 + c).reshape(-1), (d + i) * d2 + d + j]).to(self._nat1.device)
            self._pidx = idx
        return idx

    def _sync_sites(self):
        """Packed mode: take back a dense `nat2` that was edited in place since it was handed out."""
        if self._packed and self._nat2 is not None and not self._nat2_seen.matches(self._nat2):
            self.nat2 = self._nat2

    @property
    def nat2(self):
        if self._packed:
            self._sync_sites()
            if self._nat2 is None:
                d2 = self._nat1.shape[-1]
                flat = torch.zeros((self._nat2q.shape[0], d2 * d2), dtype=torch.float64, device=self._nat2q.device)
                flat[:, self._pack_index()] = self._nat2q
                low = flat.view(-1, d2, d2)
                self._nat2 = low + low.transpose(-1, -2) - torch.diag_embed(torch.diagonal(low, dim1=-2, dim2=-1))
                self._nat2_seen = Stamp(self._nat2)
        return self._nat2

    @nat2.setter
    def nat2(self, value):
        self._nat2 = value
        self._version += 1
        if self._packed:
            self._nat2_seen = Stamp(value)
            self._nat2q = value.reshape(value.shape[0], -1)[:, self._pack_index()].contiguous()

    def _sites_written(self):
        """A library call wrote the resident sites: a dense `nat2` handed out earlier is stale, and every stamp on the sites moves."""
        if self._packed:
            self._nat2 = None
        self._version += 1

    def _site_parts(self):
        self._sync_sites()
        return self._version, self._nat1, self._nat2q if self._packed else self._nat2

    def _key(self):
        """Stamp of the current sites: what every cached posterior quantity is kept for."""
        return Stamp(*self._site_parts())

    def _current(self, stamp):
        return stamp.matches(*self._site_parts())

    @property
    def kernel(self):
        return self._kernel

    @property
    def likelihood(self):
        return self._likelihood

    @property
    def dist_p(self):
        if self._dist_p is None:
            self._dist_p = self._kernel.state_space_model(self.inducing_inputs)
        return self._dist_p

    @property
    def dist_q(self):
        """Prior naturals + overlap-added site naturals (sparse_variational_cvi.py:140-174) as a StateSpaceModel."""
        p = self.dist_p
        if self._shard is not None:
            self._gather_sites()
        return self._posterior_ssm()

    def _posterior_ssm(self, nat1=None, nat2=None):
        """The posterior over the inducing states for the given sites (the model's own by default) as a StateSpaceModel."""
        p = self.dist_p
        lin, diag, sub = (x.clone() for x in self._theta(nat1, nat2))      # _theta() reuses its buffers
        q = naturals_to_ssm_params_packed(p.plan, lin, diag, sub)
        q.batch_shape = p.batch_shape
        return q

    @property
    def posterior(self):
        return ConditionalProcess(self.dist_q, self._kernel, self.inducing_inputs, self._time_mean)

    def local_objective_and_gradients(self, Fmu, Fvar, Y):
        obj = self._likelihood.variational_expectations(Fmu, Fvar, Y).sum()
        return obj, self._likelihood.ve_gradients_expectation(Fmu, Fvar, Y)

    # ---- fused route (csrc/mfgm_sparse.h): sorted data points, one chain ---------------------------------------------------------------
    _data_extra = ()          # what a data set's constants depend on besides the inputs: more parts of the stamp they are kept under

    def _data(self, input_data, keep=True):
        """Per-data-set constants of the device route (_build_data of the inputs, input_data[0]), or None where the route does not
        apply; kept until the inputs move.  keep=False (other inputs, as prediction points): the kept set serves when it is the one
        asked for, nothing is stored."""
        x = input_data[0]
        c = getattr(self, "_data_cache", None)
        if c is not None and c[0].matches(x, *self._data_extra):
            return c[1]
        val = self._build_data(x)
        if keep:
            self._data_cache = (Stamp(x, *self._data_extra), val)
        return val

    def _build_data(self, time_points):
        """The constants of the fused route, uncached: CSR offsets of the data points per inter-inducing interval, w_i = H P_i,
        c_i = H T_i H^T (conditionals.py:207-256: functions of the time points and the kernel only), the kernel's initial state; or None
        when the route does not apply (unsorted or batched time points)."""
        val = None
        z = self.inducing_inputs
        if (time_points.dim() == 1 and z.dim() == 1 and time_points.is_cuda and os.environ.get("VIDP_FUSED_SPARSE", "1") != "0"
                and (time_points.numel() < 2 or bool((time_points[1:] >= time_points[:-1]).all()))):
            M, d = int(z.shape[0]), self._kernel.state_dim
            m_lo, m_hi, own = 0, M + 1, slice(None)
            if self._shard is not None:
                # the data points of the owned intervals: a contiguous slice of the sorted time points
                m_lo, m_hi = self._m_lo, self._m_hi
                edges = torch.searchsorted(torch.searchsorted(z.contiguous(), time_points.contiguous()),
                                           torch.tensor([m_lo, m_hi], device=z.device), right=False)
                own = slice(int(edges[0]), int(edges[1]))
                time_points = time_points[own]
            N = int(time_points.shape[0])
            if N > 0:
                P, Tc, idx = _conditional_statistics(time_points, z, self._kernel)
                H = self._kernel.generate_emission_model(time_points[:1]).emission_matrix[0]      # [1, d], time-invariant
                w = (H @ P)[:, 0, :].contiguous()                                                  # [N, 2d]
                cc = (H @ Tc @ H.transpose(-1, -2))[:, 0, 0].contiguous()                          # [N]
            else:
                idx = torch.zeros(0, dtype=torch.int64, device=z.device)
                w, cc = (torch.zeros((1, 2 * d), dtype=torch.float64, device=z.device), torch.zeros(1, dtype=torch.float64, device=z.device))
            seg = csr_offsets(idx - m_lo, m_hi - m_lo)
            pm, pc = initial_state(self._kernel, z)
            sd = _lib.SparseData()
            sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = M, d, N, m_lo, m_hi
            sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = seg.data_ptr(), w.data_ptr(), cc.data_ptr(), pm.data_ptr(), pc.data_ptr()
            val = dict(struct=sd, keep=(seg, w, cc, pm, pc), N=N, own=own, t=time_points)
        if val is None and self._shard is not None:
            raise ValueError("a shared chain needs sorted, un-batched time points on the device")
        return val

    def _prior_natural(self):
        """Prior naturals in natural layout ([T, d], [T, d, d] x 2) + their packed form and sum log chol (cached: the prior is fixed)."""
        if getattr(self, "_pn", None) is None:
            p = self.dist_p
            pl = p.plan
            nat = pl.ssm_to_naturals(p.packed.A, p.packed.off, p.packed.chol, want_logdet=True)
            T, d = p.T, p.d
            if pl.d > 8:      # wide plans: the packed arrays are the natural ones
                lin, diag, sub = nat["lin"].view(T, d), nat["diag"].view(T, d, d), nat["sub"].view(T, d, d)
            else:
                lin, diag = pl.unpack(VEC, nat["lin"])[0], pl.unpack(SYM, nat["diag"])[0]
                sub = torch.zeros((T, d, d), dtype=torch.float64, device=pl.device)
                sub[:T - 1] = pl.unpack(FULL, nat["sub"], T - 1)[0]
            self._pn = dict(nat=nat, lin=lin.contiguous(), diag=diag.contiguous(), sub=sub.contiguous(), zeros=pl.zeros(VEC))
        return self._pn

    # the inverse form is used while the prior's precision blocks are conditioned better than this (tests/test_gpu_accuracy.py: at
    # 3.7e10, config 5's grid, both forms hold 1e-10 on the ELBO; at 1.1e13 the inverse form is 10-1000 x worse than the Cholesky form)
    INVERSE_FORM_MAX_COND = 1e11

    def _inverse_form(self):
        """The marginals come from the inverse-form sweeps (Plan.factor(moments_only=True), d > 8).  They lose ~10 eps cond(F_t) where
        the Cholesky form loses ~0.05 eps cond: on config 5's kernel and grid (rho = dz / lengthscale >= 0.05) the ELBO agrees with the
        oracle to 1e-10 in either form; on grids so fine that the prior precision is numerically singular (rho ~ 0.005, cond 1e15)
        neither form nor the NumPy oracle is meaningful in fp64.  So the form follows the conditioning of the prior's precision blocks
        (a sample of them, once per prior): above INVERSE_FORM_MAX_COND the Cholesky form is used, with a warning.
        VIDP_SPARSE_INVERSE_FORM=0 / 1 forces the Cholesky / inverse form."""
        if not self.dist_p.plan.wide:
            return False
        forced = os.environ.get("VIDP_SPARSE_INVERSE_FORM")
        if forced is not None:
            return forced != "0"
        pn = self._prior_natural()
        if "inverse_ok" not in pn:
            cond = self._prior_block_condition(pn["diag"])
            pn["inverse_ok"] = cond <= self.INVERSE_FORM_MAX_COND
            if not pn["inverse_ok"]:
                import warnings
                warnings.warn(f"SparseCVIGaussianProcess: the prior's precision blocks have condition number ~{cond:.1e} on this grid; "
                              "using the Cholesky-form sweeps (slower, ~200x more accurate) instead of the inverse form", RuntimeWarning)
        return pn["inverse_ok"]

    @staticmethod
    def _prior_block_condition(diag, samples=128):
        """Largest 2-norm condition number over a sample of the prior's diagonal precision blocks ([T, d, d], lower triangle valid): evenly
        spaced nodes plus both ends (on a uniform grid every interior block is the same).  Host side, once per prior."""
        T = diag.shape[0]
        idx = torch.unique(torch.cat([torch.linspace(0, T - 1, min(samples, T)).round().long(), torch.tensor([0, max(T - 2, 0), T - 1])]))
        blk = diag[idx.to(diag.device)].detach().cpu()
        low = torch.tril(blk)
        blk = low + torch.tril(blk, -1).transpose(-1, -2)
        ev = torch.linalg.eigvalsh(blk).abs()
        return float((ev.max(-1).values / ev.min(-1).values.clamp_min(1e-300)).max())

    def _fused_theta(self):
        return (self._inverse_form() and os.environ.get("VIDP_FUSED_THETA", "1") != "0" and self.nat1.is_contiguous()
                and (self._packed or self.nat2.is_contiguous()))

    def _theta(self, nat1=None, nat2=None):
        """Posterior naturals of the given sites (dense, contiguous; the model's own by default), packed (lin, diag, sub): one pass over
        the sites (mfgm_sparse_theta)."""
        nat1 = self.nat1 if nat1 is None else nat1
        nat2 = self.nat2 if nat2 is None else nat2
        p = self.dist_p
        pl, T, d = p.plan, p.T, p.d
        pn = self._prior_natural()
        wide = pl.d > 8
        b = self.__dict__.setdefault("_theta_bufs", {})
        if not b:
            mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=pl.device)
            b.update(lin=mk(T, d), diag=mk(T, d, d), sub=mk(T, d, d))
        _lib.check(pl.lib.mfgm_sparse_theta(T, d, _ptr(nat1), _ptr(nat2), _ptr(pn["lin"]), _ptr(pn["diag"]), _ptr(pn["sub"]),
                                            _ptr(b["lin"]), _ptr(b["diag"]), _ptr(b["sub"]), _stream()), "mfgm_sparse_theta")
        if wide:
            return b["lin"].view(-1), b["diag"].view(-1), b["sub"].view(-1)
        return (pl.pack(VEC, b["lin"][None]), pl.pack(SYM, b["diag"][None]),
                pl.pack(FULL, b["sub"][None, :T - 1].contiguous()) if T > 1 else pl.zeros(FULL))

    def _marginals(self):
        """Posterior marginals of the inducing states for the current sites: one factorisation + selected inverse, cached until the
        sites move.  dict(mu [T, d], Sig [T, d, d], Sub [T, d, d] natural; packed Sig / Sub / x; log|L|)."""
        m = getattr(self, "_marg", None)
        if m is not None and self._current(m["version"]):
            return m
        p = self.dist_p
        pl, T, d = p.plan, p.T, p.d
        bufs = self.__dict__.setdefault("_sweep_bufs", dict(f={}, s={}))
        if self._shard is not None:
            # one chain shared between processes: the same passes on the owned segments, one exchange (distributed.ChainShard)
            sh, pn = self._shard, self._prior_natural()
            pl = sh.plan
            f = sh.sparse_factor(self._nat1, self._nat2q if self._packed else self._nat2, pn["lin"], pn["diag"], pn["sub"], out=bufs["f"],
                                 packed=self._packed)
        elif self._fused_theta():
            # the level-0 passes of the factorisation form  prior + overlap-added sites  while loading: no posterior naturals in memory
            pn = self._prior_natural()
            f = pl.sparse_factor(self._nat1, self._nat2q if self._packed else self._nat2, pn["lin"], pn["diag"], pn["sub"], want_logdet=True,
                                 out=bufs["f"], packed=self._packed)
        else:
            lin, diag, sub = self._theta()
            f = pl.factor(diag, sub, lin, aD=-2.0, aS=-1.0, aR=1.0, want_logdet=True, out=bufs["f"], moments_only=self._inverse_form())
        bufs["f"].update(L=f["L"], G=f["G"], y=f["y"], form=f["form"])
        s = pl.selinv(f["L"], f["G"], f["y"], want_sub=True, out=bufs["s"], form=f["form"])
        bufs["s"].update(Sig=s["Sig"], Sub=s["Sub"], x=s["x"])
        if self._shard is not None:
            self._shard.left_marginal(s["Sig"], s["x"])      # the pair marginal of the first owned interval reaches one node to the left
        if pl.d > 8:
            mu, Sig, Sub = s["x"].view(T, d), s["Sig"].view(T, d, d), s["Sub"].view(T, d, d)
        else:
            mu, Sig = pl.unpack(VEC, s["x"])[0], pl.unpack(SYM, s["Sig"])[0]
            Sub = torch.zeros((T, d, d), dtype=torch.float64, device=pl.device)
            if T > 1:
                Sub[:T - 1] = pl.unpack(FULL, s["Sub"], T - 1)[0]
        self._marg = dict(version=self._key(), mu=mu, Sig=Sig, Sub=Sub, packed=s, logdetL=f["logdet"])
        return self._marg

    @staticmethod
    def _own_observations(data, observations):
        """observations[data["own"]] as ONE tensor object per (data set, observation tensor, version)."""
        c = data.get("y_own")
        if c is None or not c[0].matches(observations):
            c = data["y_own"] = (Stamp(observations), observations[data["own"]])
        return c[1]

    def _mean_at(self, data):
        """m(t) [N, 1] at the owned data points of a fused data set, kept with it (the data cache goes with the kernel)."""
        m = data.get("mean")
        if m is None:
            m = data["mean"] = self._time_mean(data["t"]).reshape(-1, 1).contiguous()
        return m

    def _predict_f_data(self, data):
        """(fmu, fvar) [N, 1] at the data points: those of the zero-mean part, the mean shifted by the mean function."""
        res = self._predict_g_data(data)
        if self._time_mean is None:
            return res
        return res[0] + self._mean_at(data), res[1]

    def _predict_g_data(self, data):
        """(fmu, fvar) [N, 1] of the zero-mean part at the data points from the cached marginals (mfgm_sparse_predict)."""
        c = getattr(self, "_pred_cache", None)
        if c is not None and self._current(c[0]) and c[1] is data:
            return c[2]          # the sites have not moved since these were computed (the ELBO of the previous iteration)
        m = self._marginals()
        pl = self.dist_p.plan if self._shard is None else self._shard.plan
        N = data["N"]
        out = torch.empty((2, max(N, 1)), dtype=torch.float64, device=pl.device)[:, :N]
        if pl.wide and (self._shard is not None or os.environ.get("VIDP_FUSED_SPARSE_KL", "1") != "0"):
            # the pass over the pair covariances also takes the trace / Mahalanobis terms of KL[q || p] (what classic_elbo asks for next)
            pn = self._prior_natural()
            kt = torch.empty(2, dtype=torch.float64, device=pl.device)
            _lib.check(pl.lib.mfgm_sparse_predict_kl(ctypes.byref(data["struct"]), _ptr(m["mu"]), _ptr(m["Sig"]), _ptr(m["Sub"]), _ptr(out[0]),
                                                     _ptr(out[1]), pl.h, _ptr(pn["nat"]["diag"]), _ptr(pn["nat"]["sub"]), -2.0, -1.0,
                                                     _ptr(self._prior_mean_packed()), _ptr(kt[0:1]), _ptr(kt[1:2]), _ptr(pl.ws), _stream()),
                       "mfgm_sparse_predict_kl")
            self._kl_cache = (self._key(), kt[0:1], kt[1:2])
        else:
            _lib.check(pl.lib.mfgm_sparse_predict(ctypes.byref(data["struct"]), _ptr(m["mu"]), _ptr(m["Sig"]), _ptr(m["Sub"]), _ptr(out[0]),
                                                  _ptr(out[1]), _stream()), "mfgm_sparse_predict")
        res = (out[0][:, None], out[1][:, None])
        self._pred_cache = (self._key(), data, res)
        return res

    def update_sites(self, input_data):
        """theta_m <- (1 - rho) theta_m + rho g_m, g_m = data gradients projected through p(f_k | v_m) (sparse_variational_cvi.py:176-221).
        In mini-batch mode (num_data=) input_data is one batch of n points in any order and g_m is the batch's sum times num_data / n.
        Unlike the reference, whose sparse variational models scale the bound only, the scale enters the site gradient too: without
        it the fixed point of the updates is the posterior of n observations, not of num_data.  A site whose interval holds no batch
        point decays."""
        if self.num_data is not None:
            return self._update_sites_batch(input_data)
        data = self._data(input_data)
        if data is None:
            return self._update_sites_generic(input_data)
        # the SAME tensor object for the owned observations every step, so that a likelihood's per-observation-tensor caches hit (a
        # fresh slice object never would)
        self._update_sites_data(data, self._own_observations(data, input_data[1]))

    def _update_sites_data(self, data, y_own, scale=None):
        """update_sites on the constants `data` of a sorted data set with the observations of its owned points; scale: the weight of
        every point's gradient (a mini-batch), None for 1."""
        fx_mus, fx_covs = self._predict_f_data(data)
        # the gradients alone: the reference's local_objective_and_gradients also returns the objective value, which update_sites drops
        # (:187-189) -- eight element-wise launches over the observations per step here
        grads = self._likelihood.ve_gradients_expectation(fx_mus, fx_covs, y_own)
        g1, g2 = grads[0].reshape(-1).contiguous(), grads[1].reshape(-1).contiguous()
        if self._time_mean is not None:
            # from the expectation parameters of f to those of g = f - m, which the sites are on: d/dmu - 2 d/dvar mu_g
            g1 = g1 + 2.0 * g2 * self._mean_at(data).reshape(-1)
        if scale is not None:
            g1, g2 = scale * g1, scale * g2
        self._site_update_launch(data["struct"], g1, g2)

    def _site_update_launch(self, struct, g1, g2):
        """sites <- (1 - rho) sites + rho sum_{i in interval} (g1_i w_i, g2_i w_i w_i^T) on the resident sites, in place."""
        pl = self.dist_p.plan
        self._sync_sites()
        if self._packed:
            _lib.check(pl.lib.mfgm_sparse_site_update_q(ctypes.byref(struct), _ptr(g1), _ptr(g2), float(self.learning_rate),
                                                        _ptr(self._nat1), _ptr(self._nat2q), _stream()), "mfgm_sparse_site_update_q")
        else:
            _lib.check(pl.lib.mfgm_sparse_site_update(ctypes.byref(struct), _ptr(g1), _ptr(g2), float(self.learning_rate),
                                                      _ptr(self._nat1), _ptr(self._nat2), _stream()), "mfgm_sparse_site_update")
        self._sites_written()
        if self._shard is not None:
            self._pass_edge_site()

    def _pass_edge_site(self):
        """A shared chain: the factorisation of the owned nodes reads the site node_hi, which the right neighbour owns and has just
        updated -- every process publishes its first owned site, one all-gather of [2d + 4d^2] doubles per process."""
        sh = self._shard
        lo, hi = sh.node_lo, sh.node_hi
        n2 = self._nat2q if self._packed else self._nat2
        mine = torch.cat([self._nat1[lo], n2[lo].reshape(-1)])
        every = sh.allgather(mine)
        if sh.rank + 1 < sh.world:
            d2 = self._nat1.shape[-1]
            self._nat1[hi].copy_(every[sh.rank + 1, :d2])
            n2[hi].copy_(every[sh.rank + 1, d2:].view(n2[hi].shape))
            self._sites_written()

    def _gather_sites(self):
        """A shared chain: the sites of every process on every process (dist_q / posterior of the whole chain; not on the training path)."""
        sh = self._shard
        self._sync_sites()
        for t in (self._nat1, self._nat2q if self._packed else self._nat2):
            own = torch.zeros_like(t)
            own[self._m_lo:self._m_hi] = t[self._m_lo:self._m_hi]
            t.copy_(sh.allreduce(own))
        self._sites_written()

    def _update_sites_generic(self, input_data, scale=None):
        time_points, observations = input_data
        fx_mus, fx_covs = self.posterior.predict_f(time_points)
        _, grads = self.local_objective_and_gradients(fx_mus, fx_covs, observations)
        if self._time_mean is not None:
            grads = (grads[0] + 2.0 * grads[1] * self._time_mean(time_points), grads[1])      # (as in update_sites)
        if scale is not None:
            grads = (scale * grads[0], scale * grads[1])                                       # (a mini-batch)
        H = self._kernel.generate_emission_model(time_points).emission_matrix
        P, _ = conditional_statistics(time_points, self.inducing_inputs, self._kernel)
        theta_linear, lik_nat2 = back_project_nats(grads[0], grads[1], H @ P)
        idx = torch.searchsorted(self.inducing_inputs.contiguous(), time_points.contiguous())
        s1 = torch.zeros_like(self.nat1).index_add_(0, idx, theta_linear)
        s2 = torch.zeros_like(self.nat2).index_add_(0, idx, lik_nat2)
        lr = self.learning_rate
        self.nat1 = (1 - lr) * self.nat1 + lr * s1      # (the setters move the stamps)
        self.nat2 = (1 - lr) * self.nat2 + lr * s2

    def classic_elbo(self, input_data):
        """sum_i E_q log p(y_i | f_i) - KL[q(s_Z) || p(s_Z)] (sparse_variational_cvi.py:270-292)."""
        if self.num_data is not None:
            return self._classic_elbo_batch(input_data)
        data = self._data(input_data)
        if data is None:
            return self._classic_elbo_generic(input_data)
        return self._classic_elbo_data(data, self._own_observations(data, input_data[1]))

    def _classic_elbo_generic(self, input_data, scale=1.0):
        time_points, observations = input_data
        q = self.dist_q
        fx_mus, fx_covs = ConditionalProcess(q, self._kernel, self.inducing_inputs, self._time_mean).predict_f(time_points)
        ve = self._likelihood.variational_expectations(fx_mus, fx_covs, observations).sum()
        if scale != 1.0:
            ve = scale * ve
        return ve - q.kl_divergence(self.dist_p).sum()

    def _classic_elbo_data(self, data, y_own, scale=1.0):
        """classic_elbo on the constants `data` of a sorted data set with the observations of its owned points; scale: the weight of
        the expectation term (a mini-batch)."""
        fx_mus, fx_covs = self._predict_f_data(data)
        ve_terms = getattr(self._likelihood, "variational_expectations_terms", None)
        kc = getattr(self, "_kl_cache", None)
        if ve_terms is not None and self._shard is None and kc is not None and self._current(kc[0]):
            # every piece of the bound is a device scalar by now: assemble  VE - KL  in one launch (a dozen scalar torch kernels otherwise),
            # NaN-poisoned when a pivot block of the factorisation was not positive definite
            m, pn, p = self._marginals(), self._prior_natural(), self.dist_p
            c, w, (t1, t2) = ve_terms(fx_mus, fx_covs, y_own)
            if scale != 1.0:
                c, w = scale * c, scale * w
            terms = torch.cat([t1, t2, kc[1].reshape(1), kc[2].reshape(1), pn["nat"]["sumlogchol"].reshape(1), m["logdetL"].reshape(1)])
            wts = (ctypes.c_double * 6)(w, w, -0.5, -0.5, -1.0, -1.0)
            out = torch.empty(1, dtype=torch.float64, device=terms.device)
            _lib.check(p.plan.lib.mfgm_combine_terms(6, 1, _ptr(terms), wts, c + 0.5 * float(p.T * p.d), None, 0.0, _ptr(p.plan.info), None,
                                                     _ptr(out), _stream()), "mfgm_combine_terms")
            return out[0]
        ve_sum = getattr(self._likelihood, "variational_expectations_sum", None)
        ve = ve_sum(fx_mus, fx_covs, y_own) if ve_sum is not None else self._likelihood.variational_expectations(fx_mus, fx_covs, y_own).sum()
        if scale != 1.0:
            ve = scale * ve
        # KL[q || p] from the marginal blocks of q and the prior's naturals (state_space_model.py:528-593); the prior mean is zero
        m, pn = self._marginals(), self._prior_natural()
        p = self.dist_p
        pl = p.plan
        s = m["packed"]
        kc = getattr(self, "_kl_cache", None)
        if self._shard is not None:
            # partial sums over the owned data points, intervals and nodes: one all-reduce of four doubles
            kc = self._kl_cache
            tot = self._shard.allreduce(torch.cat([ve.reshape(1), kc[1], kc[2], m["logdetL"].reshape(1)]))
            kl = 0.5 * (tot[1] + tot[2] - float(p.T * p.d) + 2.0 * pn["nat"]["sumlogchol"].sum() + 2.0 * tot[3])
            return tot[0] - kl
        if kc is not None and self._current(kc[0]):
            tr, mh = kc[1], kc[2]          # taken together with the predictions (mfgm_sparse_predict_kl)
        else:
            tr, mh = pl.kl_terms(s["Sig"], s["Sub"], s["x"], pn["nat"]["diag"], pn["nat"]["sub"], self._prior_mean_packed(), aD=-2.0, aS=-1.0)
        kl = 0.5 * (tr + mh - float(p.T * p.d) + 2.0 * pn["nat"]["sumlogchol"] + 2.0 * m["logdetL"])
        return ve - kl.sum()

    def _prior_mean_packed(self):
        """Marginal means of the prior chain, packed (zero for the kernel priors)."""
        if getattr(self, "_pmu", None) is None:
            p = self.dist_p
            zero = bool((p._mu0 == 0).all() and (p._b == 0).all())
            self._pmu = p.plan.zeros(VEC) if zero else p._posterior_packed()["s"]["x"]
        return self._pmu

    def loss(self, input_data):
        return -self.classic_elbo(input_data)

    # ---- mini-batch mode (num_data=; csrc/mfgm_minibatch.h) -----------------------------------------------------------
    # For a batch (t [n], y [n, 1]) of a data set of num_data points, with scale = num_data / n:
    #   update_sites:  theta_m <- (1 - rho) theta_m + rho scale sum_{i in batch and m} (g1_i w_i, g2_i w_i w_i^T); a site whose interval
    #                  holds no batch point decays.  The scale enters the site gradient too: the reference's sparse variational models
    #                  scale the bound only, and without it the fixed point of the site updates is the posterior of n observations,
    #                  not of num_data.
    #   classic_elbo:  scale sum_i E_q log p(y_i | f_i) - KL[q(s_Z) || p(s_Z)].
    # The batch is sorted in time (plumbing: torch.sort and a gather of y); nothing of it is kept beyond the step, and the constants of
    # a full data set in _data_cache stay where they are.  The native route (_batch_native) makes the whole data pass in one launch
    # from the time points alone and never looks at the data on the host; the torch route is _build_data's formulas, uncached.
    def _batch_native(self, time_points):
        from .kernels import IndependentMultiOutput, PiecewiseKernel, StationaryKernel
        k = self._kernel
        if (os.environ.get("VIDP_NATIVE_MINIBATCH", "1") == "0" or not time_points.is_cuda or time_points.dim() != 1
                or self.inducing_inputs.dim() != 1 or k.state_dim > 8 or type(self._likelihood) not in _BATCH_KINDS
                or not isinstance(k, StationaryKernel) or isinstance(k, (PiecewiseKernel, IndependentMultiOutput))):
            return False
        terms = k._terms()
        return terms is not None and len(terms) <= 8

    def _batch_sorted(self, input_data):
        """(t sorted, y in that order [n, 1], num_data / n) of a batch."""
        t, y = input_data
        if t.dim() != 1 or t.shape[0] == 0:
            raise ValueError("a mini-batch is (time_points [n], observations [n, 1]) with n >= 1")
        n = int(t.shape[0])
        ts, perm = torch.sort(t, stable=True)
        return ts.contiguous(), y.reshape(n, -1)[perm].contiguous(), self.num_data / n

    def _batch_pass(self, input_data):
        """The native data pass of a batch: dict(struct: the SparseData of the sorted batch for the site update, g1, g2, ve [n] already
        scaled, ve_sum [1], fmu, fvar [n]); kept for the same batch object while the sites do not move (the Stamp rules)."""
        t, y = input_data
        c = getattr(self, "_batch_cache", None)
        if c is not None and c["native"] and c["stamp"].matches(t, y) and self._current(c["key"]):
            return c
        ts, ys, scale = self._batch_sorted(input_data)
        k = getattr(self, "_batch_consts", None)
        if k is None:
            z = self.inducing_inputs.contiguous()
            k = self._batch_consts = dict(z=z, terms=self._kernel._terms_struct(), init=initial_state(self._kernel, z))
        z, (pm, pc) = k["z"], k["init"]
        M, d, n, dev = int(z.shape[0]), self._kernel.state_dim, int(ts.shape[0]), ts.device
        shift = None if self._time_mean is None else self._time_mean(ts).reshape(-1).contiguous()
        m = self._marginals()
        pl = self.dist_p.plan
        lik = self._likelihood
        kind = _BATCH_KINDS[type(lik)]
        param = lik.variance if kind == _lib.LIK_GAUSSIAN else lik.param
        out = torch.empty((6, n), dtype=torch.float64, device=dev)          # c, fmu, fvar, ve, g1, g2
        w = torch.empty((n, 2 * d), dtype=torch.float64, device=dev)
        ve_sum = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(int(pl.lib.mfgm_sparse_batch_workspace_doubles(n)), dtype=torch.float64, device=dev)
        seg = torch.empty(M + 2, dtype=torch.int32, device=dev)
        _lib.check(pl.lib.mfgm_sparse_batch_predict_lik(ctypes.byref(k["terms"]), M, _ptr(z), n, _ptr(ts), _ptr(shift), kind, float(param),
                                                        float(scale), _ptr(ys), _ptr(pm), _ptr(pc), _ptr(m["mu"]), _ptr(m["Sig"]),
                                                        _ptr(m["Sub"]), None, _ptr(w), *(_ptr(o) for o in out), _ptr(ve_sum), _ptr(ws),
                                                        _ptr(pl.info), _stream()), "mfgm_sparse_batch_predict_lik")
        _lib.check(pl.lib.mfgm_sparse_batch_seg(M, _ptr(z), n, _ptr(ts), _ptr(seg), _stream()), "mfgm_sparse_batch_seg")
        sd = _lib.SparseData()
        sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = M, d, n, 0, M + 1
        sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = seg.data_ptr(), w.data_ptr(), out[0].data_ptr(), pm.data_ptr(), pc.data_ptr()
        c = dict(native=True, stamp=Stamp(t, y), key=self._key(), struct=sd, keep=(seg, w, out, ts, ys, shift), fmu=out[1], fvar=out[2],
                 ve=out[3], g1=out[4], g2=out[5], ve_sum=ve_sum, scale=scale)
        self._batch_cache = c
        return c

    def _batch_torch(self, input_data):
        """The torch route's view of a batch: dict(data: _build_data of the sorted time points or None, ts, ys, scale); kept for the
        same batch object (the constants depend on the time points and the kernel only)."""
        t, y = input_data
        c = getattr(self, "_batch_cache", None)
        if c is not None and not c["native"] and c["stamp"].matches(t, y):
            return c
        ts, ys, scale = self._batch_sorted(input_data)
        c = dict(native=False, stamp=Stamp(t, y), data=self._build_data(ts), ts=ts, ys=ys, scale=scale)
        self._batch_cache = c
        return c

    def _update_sites_batch(self, input_data):
        if self._batch_native(input_data[0]):
            c = self._batch_pass(input_data)
            return self._site_update_launch(c["struct"], c["g1"], c["g2"])
        c = self._batch_torch(input_data)
        if c["data"] is None:
            return self._update_sites_generic((c["ts"], c["ys"]), scale=c["scale"])
        self._update_sites_data(c["data"], c["ys"], scale=c["scale"])

    def _classic_elbo_batch(self, input_data):
        if self._batch_native(input_data[0]):
            c = self._batch_pass(input_data)
            kl = chain_kl(self.dist_p, self._marginals(), self._prior_natural(), self._prior_mean_packed()).sum()
            return c["ve_sum"][0] - kl
        c = self._batch_torch(input_data)
        if c["data"] is None:
            return self._classic_elbo_generic((c["ts"], c["ys"]), scale=c["scale"])
        return self._classic_elbo_data(c["data"], c["ys"], scale=c["scale"])

    # ---- kernel hyper-parameters ------------------------------------------------------------------------------------
    def elbo_and_grad(self, input_data):
        """(classic_elbo(input_data), its exact gradient with respect to the kernel's hyper-parameters with the sites held fixed): the
        gradient in the structure of kernel.hyperparameter_leaves(), CPU fp64 tensors, as log_likelihood_and_grad() of the dense
        models.  What the reference's sparse notebooks get from a GradientTape over `model.loss` between two site steps.  One chain,
        every process its own: `shard=` is not covered."""
        from . import hyper
        if self.num_data is not None:
            raise NotImplementedError("elbo_and_grad on mini-batches (num_data=) is not implemented")
        if self._time_mean is not None:
            raise NotImplementedError("elbo_and_grad with a mean function is not implemented")
        hyper.precheck(self._kernel)
        if self._shard is not None:
            raise NotImplementedError("elbo_and_grad is not implemented for a chain shared between processes (shard=)")
        if self.inducing_inputs.dim() != 1:
            raise NotImplementedError("elbo_and_grad takes one chain of inducing points")
        elbo = self.classic_elbo(input_data)
        return elbo, hyper.sparse_elbo_grad(self, input_data)

    def kernel_changed(self):
        """The kernel's hyper-parameters were assigned: drop everything derived from them (the prior and its naturals, the data cache
        with w and c, the marginal, prediction and KL caches, the theta and sweep buffers).  The sites stay."""
        self._dist_p = None
        self._pn, self._pmu = None, None
        self._data_cache = None
        self._marg, self._pred_cache, self._kl_cache = None, None, None
        self._batch_consts, self._batch_cache = None, None
        self.__dict__.pop("_theta_bufs", None)
        self.__dict__.pop("_sweep_bufs", None)
        if hasattr(self._time_mean, "kernel_changed"):
            self._time_mean.kernel_changed()

    def predict_log_density(self, input_data, full_output_cov=False):
        """log p(y* | data) per point (markovflow/models/models.py:206-227): the likelihood's predict_log_density of posterior.predict_f."""
        X, Y = input_data
        f_mean, f_var = self.posterior.predict_f(X, full_output_cov=full_output_cov)
        return self._likelihood.predict_log_density(f_mean, f_var, Y)


class DenseRouteSparseCVI(SparseCVIGaussianProcess):
    """SparseCVIGaussianProcess plus what the models built on it share (sparse Power EP, the spatio-temporal, multi-latent and
    factor-analysis models).  On CPU tensors the posterior comes from a dense (M d) x (M d) inverse (pair_sites.py: small models, the
    host tests), so the objects of the whole chain need the device; on the device the pair marginals and the KL term come from the
    parent's cached marginals.  One chain: inducing points [M]."""

    @property
    def dist_p(self):
        need_device(self, "dist_p")
        return SparseCVIGaussianProcess.dist_p.fget(self)

    @property
    def dist_q(self):
        need_device(self, "dist_q")
        return SparseCVIGaussianProcess.dist_q.fget(self)

    def _pair_marginals(self):
        """Means [M + 1, 2D] and covariances [M + 1, 2D, 2D] of the pairs of consecutive inducing states (pair_sites.pair_marginals)."""
        if not on_device(self):
            return pair_marginals(self)
        m = self._marginals()
        return pair_marginals(self, (m["mu"], m["Sig"], m["Sub"][:-1]))

    def _kl(self):
        """KL[q(s_Z) || p(s_Z)]."""
        if not on_device(self):
            return dense_kl(self)
        return chain_kl(self.dist_p, self._marginals(), self._prior_natural(), self._prior_mean_packed()).sum()

    def _site_update(self, data, g1, g2, lr, dense, packed):
        """One launch of the site update on the resident sites: the entry point `packed` on nat2q, `dense` on nat2."""
        self._sync_sites()
        name, nat2 = (packed, self._nat2q) if self._packed else (dense, self._nat2)
        _lib.check(getattr(self.dist_p.plan.lib, name)(ctypes.byref(data["struct"]), _ptr(g1), _ptr(g2), lr, _ptr(self._nat1), _ptr(nat2),
                                                       _stream()), name)
        self._sites_written()

    def _step_graph(self, input_data, cache):
        """`update_sites(input_data); classic_elbo(input_data)` captured once in a HIP graph (device route): returns a callable that
        replays it and hands back the ELBO, a device scalar that every replay overwrites.  The site tensors and the sweep buffers keep
        their addresses; a replay moves the sites behind the host's back, so it bumps their stamps and drops the cached results
        (the marginals, the KL terms and the predict-lik pass kept in the attribute `cache`).  For the models whose step is
        `_predict_lik(data, Y)` and a `_site_update` of two of its results: `_SITE_UPDATE` names them and the two entry points."""
        data = self._data(input_data)
        if data is None:
            raise NotImplementedError("step_graph needs the device route: sorted, un-batched time points on the GPU")
        # warm-up: every kernel of the step has run once (a site update at lr = 0 leaves the sites as they are), no state has moved
        r = self._predict_lik(data, input_data[1])
        self.classic_elbo(input_data)
        g1, g2, dense, packed = self._SITE_UPDATE
        self._site_update(data, r[g1], r[g2], 0.0, dense, packed)

        def drop():
            self._marg = self._kl_cache = None
            setattr(self, cache, None)

        drop()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.update_sites(input_data)
            e = self.classic_elbo(input_data)
        drop()                                       # nothing ran during the capture

        def step():
            graph.replay()
            wrote(self._nat1, self._nat2q if self._packed else self._nat2)
            self._sites_written()
            self.dist_p.plan.epoch += 1
            drop()
            return e
        step.graph = graph
        return step
