"""GPU tests of posterior sampling: Plan.sample (mfgm_packed_sample) against the NumPy restatement of the contract, the native kernel
against the natural-layout route, reproducibility, the density identity, moments, reuse of stored factors, ConditionalProcess.sample_f
and the models' posteriors."""
import math

import numpy as np
import pytest
import torch

from oracle import np_btd
from tests import np_sample
from tests.helpers import random_dominant_btd

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _factor(diag, sub, r, R0=0):
    import vidp_amd as amd
    B, T, d = r.shape
    plan = amd.Plan(B, T, d, R0=R0)
    S = plan.pack(amd.FULL, dev(sub)) if sub is not None else plan.zeros(amd.FULL)
    f = plan.factor(plan.pack(amd.SYM, dev(diag)), S, plan.pack(amd.VEC, dev(r)))
    plan.check_info()
    return plan, f


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("B, T", [(1, 1), (3, 2), (1, 37), (3, 37), (3, 1000)])
def test_plan_sample_matches_restatement(d, B, T):
    rng = np.random.default_rng(100 * d + T + B)
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    r = rng.normal(size=(B, T, d))
    S = 3
    want = np_sample.sample(diag, sub, r, seed=7, s=1, S=S)[0]
    for R0 in ([0, 5, T] if T > 2 else [0]):
        plan, f = _factor(diag, sub, r, R0=R0)
        x = host(plan.sample(f, S, seed=7))
        assert x.shape == (S, B, T, d)
        assert _rel(x, want) <= 1e-10, (R0, _rel(x, want))


# ---- 3. native against the natural-layout route; 4. reproducibility -----------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 6, 8])
def test_native_matches_fallback_and_is_reproducible(d):
    from vidp_amd import sampling
    rng = np.random.default_rng(d)
    B, T = 3, 517
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    r = rng.normal(size=(B, T, d))
    plan, f = _factor(diag, sub, r, R0=11)
    x = plan.sample(f, 8, seed=99, stream=1)
    fb = sampling.fallback_sample(plan, f, 8, seed=99, stream=1)
    assert _rel(host(x), host(fb)) <= 1e-11
    assert torch.equal(x, plan.sample(f, 8, seed=99, stream=1))
    assert torch.equal(x[:3], plan.sample(f, 3, seed=99, stream=1))
    assert (x - plan.sample(f, 8, seed=100, stream=1)).abs().max() > 0.1
    assert (x - plan.sample(f, 8, seed=99, stream=2)).abs().max() > 0.1
    assert plan.sample(f, 0, seed=99).shape == (0, B, T, d)


def test_sampler_leaves_plan_workspace_alone():
    rng = np.random.default_rng(5)
    B, T, d = 2, 400, 3
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    plan, f = _factor(diag, sub, rng.normal(size=(B, T, d)), R0=7)
    ws = plan.ws.clone()
    plan.sample(f, 5, seed=1)
    torch.cuda.synchronize()
    assert torch.equal(ws, plan.ws)


# ---- 2, 5, 10: CVI-DP double-well posteriors --------------------------------------------------------------------------------------------
def _cvidp(B, T, d, R0=0, steps=2):
    import vidp_amd as amd
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    rng = np.random.default_rng(0)
    dt = 0.01
    grid = np.arange(T) * dt
    idx = np.arange(10, T - 1, 50)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.2 * rng.normal(size=(B, len(idx), d))
    m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(0.3 * np.eye(d))),
                    prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)), plan=amd.Plan(B, T, d, R0=R0))
    for _ in range(steps):
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.2)
    return m


def _density_identity(q, x, n_chains, seed, stream=1):
    """log_pdf(x) = -1/2 |eps|^2 + 1/2 log|Lambda| - T d / 2 log 2 pi on the first n_chains chains."""
    from vidp_amd.sde_utils import normal_stream
    S, B, T, d = x.shape
    lp = host(q.log_pdf(x)).reshape(S, B)
    eps = host(normal_stream(S, B * T, d, seed=seed, stream=stream)).reshape(S, B, T, d)
    logdet = host(q.log_det_precision()).reshape(B)
    want = -0.5 * (eps ** 2).sum((-1, -2)) + 0.5 * logdet[None] - 0.5 * T * d * math.log(2 * math.pi)
    np.testing.assert_allclose(lp[:, :n_chains], want[:, :n_chains], rtol=1e-10)


def test_partition_invariance_and_density_identity():
    T, d = 20000, 6
    xs = []
    for R0 in (0, T):
        q = _cvidp(1, T, d, R0=R0).dist_q
        xs.append(host(q.sample(2, seed=3)))
        if R0 == 0:
            _density_identity(q, q.sample(2, seed=3), 1, 3)
    assert _rel(xs[0], xs[1]) <= 1e-9


def test_headline_scale_draw():
    B, T, d, S = 64, 100000, 6, 4
    m = _cvidp(B, T, d, steps=1)
    q = m.dist_q
    x = q.sample(S, seed=11)
    assert x.shape == (S, B, T, d) and bool(torch.isfinite(x).all())
    _density_identity(_sub_chains(q, 2), x[:, :2].contiguous(), 2, 11)


def _sub_chains(q, n):
    """The first n chains of a state space model (log_pdf and log_det_precision of a sub-batch)."""
    from vidp_amd.state_space_model import StateSpaceModel
    return StateSpaceModel(q._mu0[:n], q._cholP0[:n], q._A[:n], q._b[:n], q._cholQ[:n])


def test_density_identity_random_precision():
    from vidp_amd.state_space_model import StateSpaceModel
    from tests.helpers import random_ssm_params
    rng = np.random.default_rng(2)
    B, T, d = 3, 300, 4
    mu0, cP0, A, b, cQ = random_ssm_params(rng, (B,), T, d)
    q = StateSpaceModel(dev(mu0), dev(cP0), dev(A), dev(b), dev(cQ))
    x = q.sample(5, seed=21)
    _density_identity(q, x, B, 21)


# ---- 6. moments ---------------------------------------------------------------------------------------------------------------------
def test_moments_match_selected_inverse():
    rng = np.random.default_rng(9)
    B, T, d, S = 2, 40, 3, 4000
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    r = rng.normal(size=(B, T, d))
    plan, f = _factor(diag, sub, r, R0=6)
    x = host(plan.sample(f, S, seed=1234))
    Ld, Ls = np_btd.cholesky(diag, sub)
    Sd, Ss = np_btd.inverse_blocks(Ld, Ls)
    mu = np_btd.solve(Ld, Ls, np_btd.solve(Ld, Ls, r), transpose_left=True)
    sd = np.sqrt(np.diagonal(Sd, axis1=-2, axis2=-1))
    assert (np.abs(x.mean(0) - mu) <= 5 * sd / math.sqrt(S)).all()
    dx = x - mu[None]
    cov = np.einsum("nbti,nbtj->btij", dx, dx) / S
    sub_cov = np.einsum("nbti,nbtj->btij", dx[:, :, 1:], dx[:, :, :-1]) / S
    scale = sd[..., :, None] * sd[..., None, :]
    # Var of a product of two jointly normal entries is at most 2 s_i^2 s_j^2
    assert (np.abs(cov - Sd) <= 5 * math.sqrt(2) * scale / math.sqrt(S)).all()
    ssc = sd[:, 1:, :, None] * sd[:, :-1, None, :]
    assert (np.abs(sub_cov - Ss) <= 5 * math.sqrt(2) * ssc / math.sqrt(S)).all()


# ---- 7. stored factors are reused; 11. errors ----------------------------------------------------------------------------------------
def _gpr(t, y, ls=0.3, var=1.5, noise=1.0):
    from vidp_amd.kernels import Matern12
    from vidp_amd.variational_cvi import GaussianProcessRegression
    return GaussianProcessRegression((dev(t), dev(y)), Matern12(lengthscale=ls, variance=var), chol_obs_covariance=dev(np.array([[noise]])))


def _cvigp(t, y):
    from vidp_amd.kernels import Matern32
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    m = CVIGaussianProcess((dev(t), dev(y)), Matern32(lengthscale=0.5, variance=1.0), Gaussian(0.1), learning_rate=1.0)
    m.update_sites()
    return m


def test_seeded_draw_keeps_the_model_factor():
    rng = np.random.default_rng(4)
    t = np.linspace(0, 3, 30)
    y = np.sin(3 * t)[:, None] + 0.1 * rng.normal(size=(30, 1))
    for q in (_cvigp(t, y).dist_q, _cvidp(2, 300, 2).dist_q, _gpr(t, y).posterior_state_space_model):
        epoch = q.plan.epoch
        x = q.sample(3, seed=5)
        assert q.plan.epoch == epoch
        assert bool(torch.isfinite(x).all())


def test_errors():
    rng = np.random.default_rng(6)
    B, T, d = 1, 50, 3
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    r = rng.normal(size=(B, T, d))
    plan, f = _factor(diag, sub, r)
    import vidp_amd as amd
    with pytest.raises(ValueError):
        plan.sample(dict(f, form=1), 2, seed=0)
    f2 = plan.factor(plan.pack(amd.SYM, dev(diag)), plan.pack(amd.FULL, dev(sub)), plan.pack(amd.VEC, dev(r)), store_G=False)
    with pytest.raises(ValueError):
        plan.sample(f2, 2, seed=0)
    with pytest.raises(ValueError):
        plan.sample(f, -1, seed=0)
    q = _gpr(np.linspace(0, 1, 10), np.zeros((10, 1))).posterior_state_space_model
    with pytest.raises(ValueError):
        q.sample(2, generator=torch.Generator(device="cuda"), seed=1)


# ---- 8. ConditionalProcess ------------------------------------------------------------------------------------------------------------
def _gpr_data(batch_shape):
    rng = np.random.default_rng(17)
    t = np.linspace(0.0, 10.0, 10)
    y = np.sin(12 * t)[:, None] + 0.1 * rng.normal(size=(10, 1))
    tile = lambda a: np.tile(a, batch_shape + tuple(1 for _ in a.shape))
    return t, y, tile


@pytest.mark.parametrize("batch_shape", [(3,), (), (2, 1)])
def test_sample_f_shapes(batch_shape):
    t, y, tile = _gpr_data(batch_shape)
    post = _gpr(tile(t), tile(y), ls=1.0, var=1.0).posterior
    future = dev(tile(np.arange(10.5, 13.0, 0.5)))
    for ss in [0, 1, 6, (10, 10), (3, 1), (0, 1), (1, 1, 1), (2, 1, 3)]:
        f = post.sample_f(future, ss, seed=2)
        want = (ss,) if isinstance(ss, int) else ss
        assert tuple(f.shape[:-2]) == tuple(want) + tuple(batch_shape)
        assert tuple(f.shape[-2:]) == (future.shape[-1], 1)
    assert post.sample_f(future, 0).numel() == 0


def _restated_sample_state(post, new_t, S, seed):
    """posterior.py:262-377 in torch on the same streams: the joint prior draw by its own recursion (tag 2), the posterior draw at
    the conditioning points (tag 1), sorted / unsorted / padded / gathered the reference's way.  One chain."""
    from vidp_amd.conditionals import conditional_statistics
    from vidp_amd.sde_utils import normal_stream
    z = post.conditioning_time_points
    M, N = z.shape[-1], new_t.shape[-1]
    joint = torch.cat([z, new_t])
    order = torch.argsort(joint, stable=True)
    prior = post.kernel.state_space_model(joint[order])
    d, T = prior.d, M + N
    eps = normal_stream(S, T, d, seed=seed, stream=2).view(S, T, d)
    A, b, cQ, m0, cP0 = prior._A[0], prior._b[0], prior._cholQ[0], prior._mu0[0], prior._cholP0[0]
    xs = torch.empty((S, T, d), dtype=torch.float64, device="cuda")
    xs[:, 0] = m0 + eps[:, 0] @ cP0.T
    for k in range(1, T):
        xs[:, k] = xs[:, k - 1] @ A[k - 1].T + b[k - 1] + eps[:, k] @ cQ[k - 1].T
    joint_s = xs[:, torch.argsort(order)]
    post_cond = post.gauss_markov_model.sample(S, seed=seed, stream=1).reshape(S, M, d)
    delta = joint_s[:, :M] - post_cond
    zero = torch.zeros_like(delta[:, :1])
    aug = torch.cat([zero, delta, zero], dim=1)
    idx = torch.searchsorted(z, new_t)
    v = torch.cat([aug[:, idx], aug[:, idx + 1]], dim=-1)
    P, _ = conditional_statistics(new_t, z, post.kernel)
    return joint_s[:, M:] - (P @ v[..., None])[..., 0]


def test_sample_state_matches_torch_restatement():
    t, y, _ = _gpr_data(())
    post = _gpr(t, y, ls=1.0, var=1.0).posterior
    new_t = dev(np.concatenate([np.arange(0.25, 10.0, 0.5), t[[0, 4, 9]], np.arange(10.5, 12.0, 0.5)]))
    new_t, _ = torch.sort(new_t)
    got = post.sample_state(new_t, 7, seed=31)
    want = _restated_sample_state(post, new_t, 7, 31)
    assert _rel(host(got), host(want)) <= 1e-10


def _mc_check(post, new_t, S=10000, seed=8, use_y=False):
    f = host(post.sample_f(new_t, S, seed=seed))
    mu, var = (host(a) for a in post.predict_f(new_t))
    mu, var = mu.reshape(f.shape[1:]), var.reshape(f.shape[1:])
    sd = np.sqrt(var)
    assert (np.abs(f.mean(0) - mu) <= 5 * sd / math.sqrt(S) + 1e-12).all()
    # Var of the sample variance of a normal: 2 s^4 / (S - 1)
    assert (np.abs(f.var(0, ddof=1) - var) <= 5 * math.sqrt(2.0 / (S - 1)) * var + 1e-12).all()


def test_sample_f_moments_match_predict_f():
    t, y, _ = _gpr_data(())
    post = _gpr(t, y, ls=1.0, var=1.0).posterior
    new_t = dev(np.concatenate([np.arange(0.0, t[-1], 0.5), np.arange(t[-1] + 0.5, 13.0, 0.5)]))
    _mc_check(post, new_t)


# ---- 9. models ----------------------------------------------------------------------------------------------------------------------
def test_gpr_posterior_predict_f_and_predict_y():
    from oracle import np_conditionals as npc, np_kernels, np_ssm
    rng = np.random.default_rng(12)
    N = 12
    t = np.linspace(0, 1, N)
    y = (np.cos(20 * t) + rng.normal(size=N)).reshape(-1, 1)
    m = _gpr(t, y, ls=0.3, var=1.5, noise=0.7)
    post = m.posterior
    q = post.gauss_markov_model
    oq = np_ssm.StateSpaceModel(host(q._mu0[0]), host(q._cholP0[0]), host(q._A[0]), host(q._b[0]), host(q._cholQ[0]))
    tn = np.sort(rng.uniform(-0.2, 1.2, size=7))
    mu, var = post.predict_f(dev(tn))
    omu, ovar = npc.predict_f(oq, np_kernels.Matern12(lengthscale=0.3, variance=1.5), t, tn)
    np.testing.assert_allclose(host(mu), omu, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(host(var), ovar, rtol=1e-9, atol=1e-12)
    ym, yv = post.predict_y(dev(tn))
    np.testing.assert_allclose(host(ym), host(mu), rtol=0, atol=0)
    np.testing.assert_allclose(host(yv), host(var) + 0.49, rtol=1e-14)
    ym, yc = post.predict_y(dev(tn), full_output_cov=True)
    np.testing.assert_allclose(host(yc)[..., 0, 0], host(var)[..., 0] + 0.49, rtol=1e-12)


def test_cvigp_posterior_sample_f_moments():
    rng = np.random.default_rng(13)
    t = np.linspace(0, 3, 30)
    y = np.sin(3 * t)[:, None] + 0.1 * rng.normal(size=(30, 1))
    post = _cvigp(t, y).posterior
    _mc_check(post, dev(np.concatenate([np.arange(0.05, 3.0, 0.3), [3.4, 4.0]])))


def test_sparse_cvi_posterior_sample_f_moments():
    """d = 16 (a sum of eight Matern-3/2 kernels): the natural-layout route."""
    from vidp_amd.kernels import Matern32, Sum
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    rng = np.random.default_rng(14)
    k = Sum([Matern32(lengthscale=0.3 + 0.1 * i, variance=1.0 / 8) for i in range(8)])
    z = np.linspace(0, 2, 20)
    m = SparseCVIGaussianProcess(k, dev(z), Gaussian(0.05), learning_rate=1.0)
    assert m.dist_q.d > 8
    x = np.sort(rng.uniform(0, 2, 40))
    yy = np.sin(4 * x)[:, None] + 0.2 * rng.normal(size=(40, 1))
    m.update_sites((dev(x), dev(yy)))
    _mc_check(m.posterior, dev(np.array([0.05, 0.55, 1.3, 1.95, 2.3])), S=4000)
