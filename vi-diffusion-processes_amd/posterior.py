"""
Host-side mirror of markovflow/posterior.py `ConditionalProcess` and `AnalyticPosteriorProcess` (posterior.py:166-468): the posterior
process q(s(.)) = int p(s(.) | s(Z)) q(s(Z)) ds(Z) evaluated at arbitrary sorted time points, its marginals and its seeded samples.
"""

import os

from .conditionals import conditional_predict, pairwise_marginals


class ConditionalProcess:
    def __init__(self, posterior_dist, kernel, conditioning_time_points, mean_function=None):
        self.gauss_markov_model = posterior_dist
        self.kernel = kernel
        self.conditioning_time_points = conditioning_time_points
        self.mean_function = mean_function

    def predict_state(self, new_time_points):
        """posterior.py:207-229.  One chain, 1-d query points: the pair gather and P S P^T run in one HIP kernel per query set
        (mfgm_cond_predict) on the marginal blocks of the posterior; otherwise the batched torch route."""
        q = self.gauss_markov_model
        if (new_time_points.dim() == 1 and self.conditioning_time_points.dim() == 1 and tuple(q.batch_shape) == () and new_time_points.is_cuda
                and q.d <= 32 and os.environ.get("VIDP_FUSED_PREDICT", "1") != "0"):
            return self._predict_state_fused(new_time_points)
        pw_mu, pw_cov = pairwise_marginals(q, self.kernel.initial_mean(q.batch_shape),
                                            self.kernel.initial_covariance(self.conditioning_time_points[..., :1]))
        return conditional_predict(new_time_points, self.conditioning_time_points, self.kernel, pw_mu, pw_cov)

    def _predict_state_fused(self, new_time_points):
        import torch
        from . import _lib
        from ._lib import FULL, SYM, VEC
        from .conditionals import _conditional_statistics
        from .packed import _ptr, _stream
        q = self.gauss_markov_model
        pl, T, d = q.plan, q.T, q.d
        P, Tc, idx = _conditional_statistics(new_time_points, self.conditioning_time_points, self.kernel)
        s = q._posterior_packed()["s"]
        if pl.d > 8:          # wide plans: the packed arrays are the natural ones
            mu, Sig, Sub = s["x"].view(T, d), s["Sig"].view(T, d, d), s["Sub"].view(T, d, d)
        else:
            mu, Sig = pl.unpack(VEC, s["x"])[0], pl.unpack(SYM, s["Sig"])[0]
            Sub = torch.zeros((T, d, d), dtype=torch.float64, device=pl.device)
            if T > 1:
                Sub[:T - 1] = pl.unpack(FULL, s["Sub"], T - 1)[0]
        N = int(new_time_points.shape[0])
        dev = new_time_points.device
        pm = self.kernel.initial_mean(()).to(dev, torch.float64).contiguous()
        pc = self.kernel.initial_covariance(self.conditioning_time_points[:1]).to(dev, torch.float64).contiguous()
        mean = torch.empty((N, d), dtype=torch.float64, device=dev)
        cov = torch.empty((N, d, d), dtype=torch.float64, device=dev)
        idx32 = idx.to(torch.int32).contiguous()
        _lib.check(pl.lib.mfgm_cond_predict(T, d, N, _ptr(idx32), _ptr(P.contiguous()), _ptr(Tc.contiguous()), _ptr(pm), _ptr(pc),
                                            _ptr(mu.contiguous()), _ptr(Sig.contiguous()), _ptr(Sub.contiguous()), _ptr(mean), _ptr(cov),
                                            _stream()), "mfgm_cond_predict")
        return mean, cov

    def predict_f(self, new_time_points, full_output_cov=False):
        """posterior.py:231-260 (zero mean function unless one is supplied)."""
        em = self.kernel.generate_emission_model(new_time_points)
        m, S = self.predict_state(new_time_points)
        f, fc = em.project_state_to_f(m), em.project_state_covariance_to_f(S, full_output_cov)
        if self.mean_function is not None:
            f = f + self.mean_function(new_time_points)
        return f, fc

    def sample_state_trajectories(self, new_time_points, sample_shape, *, input_data=None, seed=0):
        """posterior.py:262-377: (samples at new_time_points, samples at the conditioning points), shapes
        sample_shape + batch_shape + [N, d] and sample_shape + batch_shape + [M, d].  `input_data` is ignored, as in the reference.

        The prior is drawn jointly at the sorted union of the time points (stream tag 2), ancestrally through the prior's
        state space form -- a new point that coincides with a conditioning point has a zero-length transition there, whose precision
        does not exist -- and the posterior at the conditioning points from its factor (tag 1, include/mfgm.h).  Then
        s_new = s_prior - P [delta_-, delta_+],  delta = prior - posterior at the conditioning points, zero-padded at both ends."""
        import torch
        from .conditionals import conditional_statistics
        from .sampling import POSTERIOR_STREAM, PRIOR_STREAM, sample_shape_tuple
        sshape, S = sample_shape_tuple(sample_shape)
        q = self.gauss_markov_model
        bs, d = tuple(q.batch_shape), q.d
        z, t = self.conditioning_time_points, new_time_points
        M, N = int(z.shape[-1]), int(t.shape[-1])
        if S == 0:
            empty = lambda n: torch.zeros(sshape + bs + (n, d), dtype=torch.float64, device=t.device)
            return empty(N), empty(M)
        joint = torch.cat([z, t], dim=-1)
        sort_ind = torch.argsort(joint, dim=-1, stable=True)
        prior = self.kernel.state_space_model(torch.gather(joint, -1, sort_ind))
        xs = _ancestral_sample(prior, S, seed, PRIOR_STREAM)                       # [S, Bp, M + N, d]
        Bp = xs.shape[1]
        unsort = torch.argsort(sort_ind, dim=-1).reshape(-1, M + N)                  # [Bp, M + N]
        xs = torch.gather(xs, 2, unsort[None, :, :, None].expand(S, Bp, M + N, d))
        prior_cond, prior_new = xs[:, :, :M], xs[:, :, M:]
        post_cond = q.sample(S, seed=seed, stream=POSTERIOR_STREAM).reshape(S, q.B, M, d)
        delta = prior_cond - post_cond                                               # [S, B, M, d]
        B = delta.shape[1]
        zero = torch.zeros_like(delta[:, :, :1])
        aug = torch.cat([zero, delta, zero], dim=2)
        idx = torch.searchsorted(z.contiguous(), t.contiguous()).reshape(-1, N)
        idx = idx.expand(B, N) if idx.shape[0] != B else idx
        u_minus = torch.gather(aug, 2, idx[None, :, :, None].expand(S, B, N, d))
        u_plus = torch.gather(aug, 2, (idx + 1)[None, :, :, None].expand(S, B, N, d))
        v = torch.cat([u_minus, u_plus], dim=-1)
        P, _ = conditional_statistics(t, z, self.kernel)
        P = P.reshape(-1, N, d, 2 * d)
        new = prior_new - (P[None] @ v[..., None])[..., 0]
        return new.reshape(sshape + bs + (N, d)), post_cond.reshape(sshape + bs + (M, d))

    def sample_state(self, new_time_points, sample_shape, *, input_data=None, seed=0):
        """posterior.py:379-389."""
        return self.sample_state_trajectories(new_time_points, sample_shape, input_data=input_data, seed=seed)[0]

    def sample_f(self, new_time_points, sample_shape, *, input_data=None, seed=0):
        """posterior.py:391-411: H s + mean function, shape sample_shape + batch_shape + [N, output_dim]."""
        s = self.sample_state(new_time_points, sample_shape, input_data=input_data, seed=seed)
        f = self.kernel.generate_emission_model(new_time_points).project_state_to_f(s)
        if self.mean_function is not None:
            f = f + self.mean_function(new_time_points)
        return f


def _ancestral_sample(ssm, S, seed, stream):
    """[S, B, T, d] draws of a state space model by its own recursion x_0 = mu0 + chol P0 eps_0, x_{k+1} = A_k x_k + b_k + chol Q_k eps_k
    (the reference's StateSpaceModel.sample), with eps from the normal stream (index rule of include/mfgm.h) and the solve against the
    unit lower block-bidiagonal A^{-1} on the device.  Zero process covariances are allowed."""
    import torch
    from .block_tri_diag import LowerTriangularBlockTriDiagonal
    from .sampling import check_seed
    from .sde_utils import normal_stream
    seed, stream = check_seed(seed, stream)
    B, T, d = ssm.B, ssm.T, ssm.d
    dev = ssm._A.device
    if S == 0:
        return torch.zeros((0, B, T, d), dtype=torch.float64, device=dev)
    eps = normal_stream(S, B * T, d, seed=seed, stream=stream, device=dev).view(S, B, T, d)
    chols = torch.cat([ssm._cholP0[:, None], ssm._cholQ], dim=1)
    off = torch.cat([ssm._mu0[:, None, :], ssm._b], dim=1)
    z = (chols[None] @ eps[..., None])[..., 0] + off[None]
    if T == 1:
        return z
    eye = torch.eye(d, dtype=torch.float64, device=dev).expand(S * B, T, d, d).contiguous()
    negA = (-ssm._A)[None].expand(S, B, T - 1, d, d).reshape(S * B, T - 1, d, d).contiguous()
    return LowerTriangularBlockTriDiagonal(eye, negA).solve(z.reshape(S * B, T, d)).reshape(S, B, T, d)


class AnalyticPosteriorProcess(ConditionalProcess):
    """posterior.py:414-468: a ConditionalProcess that also knows the likelihood, for predict_y."""

    def __init__(self, posterior_dist, kernel, conditioning_time_points, likelihood, mean_function=None):
        super().__init__(posterior_dist, kernel, conditioning_time_points, mean_function)
        self.likelihood = likelihood

    def predict_y(self, new_time_points, full_output_cov=False):
        """posterior.py:443-468: the likelihood's predict_mean_and_var of predict_f."""
        return self.likelihood.predict_mean_and_var(*self.predict_f(new_time_points, full_output_cov=full_output_cov))
