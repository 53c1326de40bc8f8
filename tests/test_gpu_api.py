"""
GPU parity tests of the reference-named host classes (StateSpaceModel, block_tri_diag, the SSM <-> eta/theta
transformations, CVISitesSSM) against the NumPy oracle.  fp64; tolerance 1e-6 relative (north-star: 1e-5).
"""
import os

import numpy as np
import pytest

from oracle import np_btd, np_models, np_ssm, np_transforms
from tests.helpers import assert_close, random_dominant_btd, random_spd_btd, random_ssm_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.detach().cpu().numpy()


@pytest.mark.parametrize("d,T", [(1, 2), (3, 4), (5, 6), (3, 70)])
def test_state_space_model(amd, rng, batch_shape, d, T):
    from vidp_amd.state_space_model import StateSpaceModel
    prm = random_ssm_params(rng, batch_shape, T, d)
    o = np_ssm.StateSpaceModel(*prm)
    g = StateSpaceModel(*[dev(p) for p in prm])
    od, os_ = o.precision()
    gp = g.precision
    assert_close(host(gp.block_diagonal), od)
    assert_close(host(gp.block_sub_diagonal), os_)
    assert_close(host(g.marginal_means), o.marginal_means)
    assert_close(host(g.marginal_covariances), o.marginal_covariances)
    assert_close(host(g.subsequent_covariances()), o.subsequent_covariances(o.marginal_covariances))
    assert_close(host(g.log_det_precision()), o.log_det_precision())
    prm2 = random_ssm_params(rng, batch_shape, T, d)
    o2 = np_ssm.StateSpaceModel(*prm2)
    g2 = StateSpaceModel(*[dev(p) for p in prm2], plan=g.plan)
    assert_close(host(g.kl_divergence(g2)), o.kl_divergence(o2), rtol=1e-6)
    np.testing.assert_allclose(host(g.kl_divergence(g)), 0.0, atol=1e-6)


def test_zero_transitions(amd):
    import torch
    from vidp_amd.state_space_model import StateSpaceModel
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        StateSpaceModel(z(2), z(2, 2), z(0, 2, 2), z(0, 2), z(0, 2, 2))


@pytest.mark.parametrize("d,T", [(1, 1), (1, 4), (3, 1), (3, 4), (2, 4), (3, 5)])
@pytest.mark.parametrize("with_sub", [True, False])
def test_block_tri_diag(amd, rng, batch_shape, d, T, with_sub):
    """Mirrors the reference's tests/unit/test_block_tri_diag.py (KA1)."""
    from vidp_amd.block_tri_diag import LowerTriangularBlockTriDiagonal, SymmetricBlockTriDiagonal
    diag, sub, Ld0, Ls0 = random_spd_btd(rng, batch_shape, T, d, with_sub)
    sym = SymmetricBlockTriDiagonal(dev(diag), None if sub is None else dev(sub))
    dense = np_btd.to_dense(diag, sub)
    assert_close(host(sym.to_dense()), dense)
    chol = sym.cholesky
    Ld, Ls = np_btd.cholesky(diag, sub)
    assert_close(host(chol.block_diagonal), Ld)
    if Ls is not None:
        assert_close(host(chol.block_sub_diagonal), Ls)
    assert_close(host(chol.abs_log_det()), 0.5 * np.linalg.slogdet(dense)[1])
    Sd, _ = np_btd.inverse_blocks(Ld, Ls)
    assert_close(host(chol.block_diagonal_of_inverse()), Sd)
    x = rng.normal(size=batch_shape + (T, d))
    low = LowerTriangularBlockTriDiagonal(dev(Ld0), None if Ls0 is None else dev(Ls0))
    for tr in (False, True):
        assert_close(host(low.solve(dev(x), transpose_left=tr)), np_btd.solve(Ld0, Ls0, x, tr), rtol=1e-5)
        assert_close(host(low.dense_mult(dev(x), transpose_left=tr)), np_btd.dense_mult(Ld0, Ls0, x, False, tr))
    assert_close(host(sym.dense_mult(dev(x))), np_btd.dense_mult(diag, sub, x, True))
    assert_close(host(low.block_diagonal_of_inverse()), np_btd.inverse_blocks(Ld0, Ls0)[0], rtol=1e-5)
    both = sym + sym
    assert_close(host(both.block_diagonal), 2 * diag)


@pytest.mark.parametrize("d,T", [(2, 33), (5, 200), (12, 97), (20, 65)])
def test_lower_block_bidiagonal_solve_direct(amd, rng, d, T):
    """LowerTriangularBlockTriDiagonal.solve (block_tri_diag.py:339-351) across several segments of the affine-recurrence
    parallelisation, both orientations, against the dense triangular solve; and on an ill-conditioned factor (cond(L) ~ 1e7,
    so cond(L L^T) ~ 1e14), where a route through the Gram matrix would lose all accuracy."""
    from vidp_amd.block_tri_diag import LowerTriangularBlockTriDiagonal
    B = 2
    for scale in (1.0, 1e-7):
        Ld = np.tril(rng.normal(size=(B, T, d, d))) * 0.3 / np.sqrt(d)
        idx = np.arange(d)
        Ld[..., idx, idx] = rng.uniform(0.8, 1.5, size=(B, T, d))
        Ld[:, T // 2, 0, 0] *= scale                  # one tiny pivot
        Ls = 0.3 / np.sqrt(d) * rng.normal(size=(B, T - 1, d, d))      # a contracting recurrence, as a Cholesky factor's is
        x = rng.normal(size=(B, T, d))
        low = LowerTriangularBlockTriDiagonal(dev(Ld), dev(Ls))
        for tr in (False, True):
            got = host(low.solve(dev(x), transpose_left=tr))
            for b in range(B):
                dense = np_btd.to_dense(Ld[b], Ls[b], symmetric=False)
                want = np.linalg.solve(dense.T if tr else dense, x[b].reshape(-1)).reshape(T, d)
                # backward-stable substitution: the residual is at rounding level whatever the conditioning
                res = (dense.T if tr else dense) @ got[b].reshape(-1) - x[b].reshape(-1)
                assert np.abs(res).max() <= 1e-9 * max(1.0, np.abs(got[b]).max())
                assert_close(got[b], want, rtol=1e-6)


def test_not_positive_definite(amd):
    import torch
    from vidp_amd.block_tri_diag import SymmetricBlockTriDiagonal
    diag = -torch.eye(2, dtype=torch.float64, device="cuda").expand(3, 2, 2).contiguous()
    with pytest.raises(ArithmeticError):
        SymmetricBlockTriDiagonal(diag).cholesky


def test_transformations(amd, rng, batch_shape):
    from vidp_amd import ssm_gaussian_transformations as tr
    from vidp_amd.state_space_model import StateSpaceModel
    prm = random_ssm_params(rng, batch_shape, 9, 3)
    o = np_ssm.StateSpaceModel(*prm)
    g = StateSpaceModel(*[dev(p) for p in prm])
    for a, b in zip(tr.ssm_to_expectations(g), np_transforms.ssm_to_expectations(o)):
        assert_close(host(a), b)
    for a, b in zip(tr.ssm_to_naturals(g), np_transforms.ssm_to_naturals(o)):
        assert_close(host(a), b)
    for a, b in zip(tr.ssm_to_naturals_no_smoothing(g), np_transforms.ssm_to_naturals_no_smoothing(o)):
        assert_close(host(a), b)
    ref = (o.A, o.b, o.cholP0, o.cholQ, o.mu0)
    for fwd, bwd in ((tr.ssm_to_expectations, tr.expectations_to_ssm_params), (tr.ssm_to_naturals, tr.naturals_to_ssm_params),
                     (tr.ssm_to_naturals_no_smoothing, tr.naturals_to_ssm_params_no_smoothing)):
        back = bwd(*fwd(g))
        for a, b in zip(back, ref):
            assert_close(host(a), b)


@pytest.mark.parametrize("d,B,T", [(1, 1, 60), (2, 3, 45), (3, 2, 130)])
def test_cvi_sites_ssm(amd, rng, d, B, T):
    """CVISitesSSM (linear prior): data-site / Girsanov-site updates and classic_elbo against the oracle, per chain."""
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.state_space_model import StateSpaceModel
    from vidp_amd.variational_cvi_sde import CVISitesSSM
    prm = random_ssm_params(rng, (B,), T, d)
    grid = np.arange(T) * 0.01
    idx = np.sort(rng.choice(T, size=7, replace=False))
    y = rng.normal(size=(B, 7, d))
    cholR = 0.4 * np.eye(d) + 0.05 * np.tril(rng.normal(size=(d, d)), -1)
    import vidp_amd
    plan = vidp_amd.Plan(B, T, d, R0=8, Rup=4)
    g = CVISitesSSM(StateSpaceModel(*[dev(p) for p in prm], plan=plan), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)))
    os_ = [np_models.CVISitesSSM(np_ssm.StateSpaceModel(*[p[b] for p in prm]), grid, idx, y[b], np_models.MultivariateGaussianLik(cholR))
           for b in range(B)]
    for it, (lr_d, lr_g) in enumerate(((1.0, 1.0), (0.5, 0.3), (0.7, 0.9))):
        g.update_data_sites(lr_d)
        g.update_girsanov_sites(lr_g)
        e = host(g.classic_elbo_per_trajectory())
        for b, o in enumerate(os_):
            o.update_data_sites(lr_d)
            o.update_girsanov_sites(lr_g)
            np.testing.assert_allclose(e[b], o.classic_elbo(), rtol=1e-6, atol=1e-6)
        mu = host(g.fx_mus)
        cov = host(g.fx_covs)
        for b, o in enumerate(os_):
            assert_close(mu[b], o.fx_mus)
            assert_close(cov[b], o.fx_covs)
    q = g.dist_q
    oq = os_[0].dist_q
    assert_close(host(q.state_transitions)[0], oq.A)
    assert_close(host(q.cholesky_process_covariances)[0], oq.cholQ)
    assert_close(host(q.state_offsets)[0], oq.b)


@pytest.mark.parametrize("d,kind", [(1, "dw"), (2, "dw"), (2, "ou"), (3, "dw"), (6, "dw"), (6, "ou"), (8, "dw")])
def test_sde_kl_kernel(amd, rng, d, kind):
    """Closed-form KL[q || p_SDE] and d KL / d eta (HIP) against the oracle's closed form, itself pinned to the reference's
    quadrature formulation in tests/test_oracle_sde.py."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    B, T, dt = 3, 37, 0.05
    qd = 0.5 + rng.random(d)
    osde = np_sde.OrnsteinUhlenbeckSDE(0.8, np.diag(qd)) if kind == "ou" else np_sde.DoubleWellSDE(np.diag(qd))
    gs = gsde.OrnsteinUhlenbeckSDE(0.8, torch.from_numpy(np.diag(qd))) if kind == "ou" else gsde.DoubleWellSDE(torch.from_numpy(np.diag(qd)))
    prm = random_ssm_params(rng, (B,), T, d, scale_A=0.8)
    init_mu, init_cov = 0.1 * rng.normal(size=d), 0.7 * np.eye(d) + 0.1 * np.ones((d, d))
    plan = amd.Plan(B, T, d, R0=5, Rup=3)
    mus, covs, subs = [], [], []
    for b in range(B):
        q = np_ssm.StateSpaceModel(*[p[b] for p in prm])
        mu, cov = q.marginals
        mus.append(mu); covs.append(cov); subs.append(q.subsequent_covariances(cov))
    mu, cov, sub = np.stack(mus), np.stack(covs), np.stack(subs)
    pm, pc, ps = plan.pack(amd.VEC, dev(mu)), plan.pack(amd.SYM, dev(cov)), plan.pack(amd.FULL, dev(sub))
    cprm = gs.params(dt, init_mu, init_cov)
    grads = (plan.empty(amd.VEC), plan.empty(amd.SYM), plan.empty(amd.FULL))
    kl0 = host(plan.sde_kl(cprm, pm, pc, ps, mode=0))
    kl1 = host(plan.sde_kl(cprm, pm, pc, ps, mode=1, grads=grads))
    plan.check_info()
    g1, gd, gsub = host(plan.unpack(amd.VEC, grads[0])), host(plan.unpack(amd.SYM, grads[1])), host(plan.unpack(amd.FULL, grads[2], T - 1))
    al, be = osde.cubic(dt)
    for b in range(B):
        kl, (o1, od, os_) = np_sde.sde_ssm_kl_closed_form(mu[b], cov[b], sub[b], al, be, qd, dt, init_mu, init_cov)
        np.testing.assert_allclose(kl0[b], kl, rtol=1e-9)
        np.testing.assert_allclose(kl1[b], kl, rtol=1e-9)
        assert_close(g1[b], o1)
        assert_close(gd[b], od)
        assert_close(gsub[b], os_)


@pytest.mark.parametrize("d,kind,B,T", [(1, "ou", 1, 60), (1, "dw", 2, 50), (2, "dw", 2, 45), (6, "dw", 2, 150), (6, "ou", 3, 67),
                                        (4, "dw", 2, 70), (5, "ou", 2, 61), (7, "dw", 1, 50), (8, "ou", 2, 45), (3, "dw+ends", 2, 41)])
def test_cvi_sites_sde(amd, rng, d, kind, B, T):
    """CVISitesSDE (CVI-DP): linearised prior, data-site and Girsanov updates, ELBO, re-linearisation, per trajectory.
    d = 6 is the bench's state dimension (ragged partition: T is not a multiple of the segment length); there the oracle takes
    its expectations from the cubic's Gaussian moments (closed_form, pinned to the reference's quadrature route at d <= 2 in
    tests/test_oracle_models.py -- the 20^6-point grid itself is out of reach).  "+ends": the first and the last node of the chain
    are observed (node 0 is where the data site and P0^{-1} meet in one block)."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    kind, _, ends = kind.partition("+")
    dt = 0.02
    qd = np.ones(d)
    osde = np_sde.OrnsteinUhlenbeckSDE(1.2, np.diag(qd)) if kind == "ou" else np_sde.DoubleWellSDE(np.diag(qd))
    gs = gsde.OrnsteinUhlenbeckSDE(1.2, torch.from_numpy(np.diag(qd))) if kind == "ou" else gsde.DoubleWellSDE(torch.from_numpy(np.diag(qd)))
    grid = np.arange(T) * dt
    idx = np.sort(rng.choice(np.arange(1, T), size=6, replace=False))
    if ends:
        idx[0], idx[-1] = 0, T - 1
    y = np.sign(rng.normal(size=(B, 6, d))) + 0.2 * rng.normal(size=(B, 6, d))
    cholR = 0.3 * np.eye(d) + (0.1 * np.eye(d, k=-1) if d > 2 else 0.0)     # d = 6: full d x d data sites, as in the bench
    init = (np.zeros(d), 0.5 * np.eye(d))
    plan = amd.Plan(B, T, d, R0=8, Rup=3)
    g = CVISitesSDE(gs, grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)), prior_initial_state=init, plan=plan)
    os_ = [np_models.CVISitesSDE(osde, grid, idx, y[b], np_models.MultivariateGaussianLik(cholR), *init, closed_form=d > 2)
           for b in range(B)]
    assert_close(host(g.dist_p.state_transitions)[0], os_[0].dist_p.A)
    assert_close(host(g.dist_p.state_offsets)[0], os_[0].dist_p.b)
    for outer in range(2):
        for lr_d, lr_g in ((0.5, 0.2), (0.3, 0.1)):
            g.update_data_sites(lr_d)
            g.update_girsanov_sites(lr_g)
            e = host(g.classic_elbo_per_trajectory())
            for b, o in enumerate(os_):
                o.update_data_sites(lr_d)
                o.update_girsanov_sites(lr_g)
                np.testing.assert_allclose(e[b], o.classic_elbo(), rtol=1e-6, atol=1e-6)
        mu, cov = host(g.fx_mus), host(g.fx_covs)
        for b, o in enumerate(os_):
            assert_close(mu[b], o.fx_mus)
            assert_close(cov[b], o.fx_covs)
        # the lean (moment-array) KL equals the full-block transition-wise KL, and the implied gradient theta_q - theta~
        # equals the full-block gradient
        np.testing.assert_allclose(host(g.KL_q_p()), host(g.KL_q_p_full()), rtol=1e-9)
        # re-linearise on the current posterior and transform the Girsanov sites (posterior unchanged)
        g.relinearize()
        for o in os_:
            o.relinearize()
        e = host(g.classic_elbo_per_trajectory())
        for b, o in enumerate(os_):
            np.testing.assert_allclose(e[b], o.classic_elbo(), rtol=1e-6, atol=1e-6)
        assert_close(host(g.dist_p.state_transitions)[B - 1], os_[B - 1].dist_p.A)
        assert_close(host(g.dist_p.state_offsets)[B - 1], os_[B - 1].dist_p.b)


@pytest.mark.parametrize("name", ["m12", "ou", "m32", "m52", "sum"])
def test_kernels_state_space_model(amd, rng, name, batch_shape):
    """Kernel -> SSM against the oracle kernels (pinned to the reference's expm test objects, KA6)."""
    from oracle import np_kernels
    from vidp_amd import kernels as K
    mk = {"m12": (lambda m: m.Matern12(0.7, 1.3)), "ou": (lambda m: m.OrnsteinUhlenbeck(1.4, 0.9)),
          "m32": (lambda m: m.Matern32(2.1, 0.4)), "m52": (lambda m: m.Matern52(0.6, 1.7)),
          "sum": (lambda m: m.Sum([m.Matern52(0.5, 1.0), m.Matern32(1.5, 0.3), m.Matern12(0.8, 2.0)], jitter=1e-9))}[name]
    gk, ok = mk(K), mk(np_kernels)
    t = np.cumsum(rng.exponential(0.2, size=batch_shape + (23,)), axis=-1)
    g, o = gk.state_space_model(dev(t)), ok.state_space_model(t)
    assert_close(host(g.state_transitions), o.A)
    assert_close(host(g.state_offsets), o.b)
    # Q = Pinf - A Pinf A^T cancels ~7 digits at small time steps: compare Q itself tightly, its Cholesky factor loosely
    gc = host(g.cholesky_process_covariances)
    assert_close(gc @ np.swapaxes(gc, -1, -2), o.cholQ @ np.swapaxes(o.cholQ, -1, -2), rtol=1e-6)
    assert_close(gc, o.cholQ, rtol=1e-4, scale_atol=1e-6)
    assert_close(host(g.cholesky_initial_covariance), o.cholP0)
    assert_close(host(g.initial_mean), o.mu0)
    np.testing.assert_allclose(gk.steady_state_covariance.numpy(), ok.steady_state_covariance(), rtol=1e-12)
    np.testing.assert_allclose(gk.feedback_matrix.numpy(), ok.feedback_matrix(), rtol=1e-12)
    H = host(gk.generate_emission_model(dev(t)).emission_matrix)
    np.testing.assert_allclose(H, ok.emission_matrix(t))


def _gpu_ssm_from_golden(g, bs, T):
    from vidp_amd.state_space_model import StateSpaceModel
    d = g["A"].shape[-1]
    bc = lambda a, shp: dev(np.broadcast_to(a, shp).copy())
    return StateSpaceModel(bc(g["mu0"], bs + (d,)), bc(g["cholP0"], bs + (d, d)), bc(g["A"], bs + (T - 1, d, d)),
                           bc(g["b"], bs + (T - 1, d)), bc(g["cholQ"], bs + (T - 1, d, d)))


@pytest.mark.parametrize("tag,bs", [("b0", ()), ("b3", (3,)), ("b21", (2, 1))])
def test_kalman_filter_golden(amd, tag, bs):
    """KA2: the reference's tests/integration/test_kalman_filter.py against ITS NumPy filter + RTS smoother (golden vectors)."""
    from tests.conftest import golden
    from vidp_amd.emission_model import EmissionModel
    from vidp_amd.kalman_filter import KalmanFilter
    g = golden(f"kalman_filter_{tag}.npz")
    T = g["y"].shape[-2]
    ssm = _gpu_ssm_from_golden(g, bs, T)
    H = dev(np.broadcast_to(g["H"], bs + (T,) + g["H"].shape).copy())
    kf = KalmanFilter(ssm, EmissionModel(H), dev(g["y"]), dev(np.linalg.cholesky(g["R"])))
    np.testing.assert_allclose(float(kf.log_likelihood()), g["log_lik_total"], rtol=1e-7)
    post = kf.posterior_state_space_model()
    assert_close(host(post.marginal_means), g["smooth_means"])
    assert_close(host(post.marginal_covariances), np.broadcast_to(g["smooth_covs"], bs + g["smooth_covs"].shape))


def test_kalman_filter_sites_golden(amd):
    """KA3: per-step Gaussian sites (tests/integration/test_kalman_filter_with_sites.py fixture)."""
    from tests.conftest import golden
    from vidp_amd.emission_model import EmissionModel
    from vidp_amd.kalman_filter import GaussianSitesNat, KalmanFilterWithSites
    g = golden("kalman_filter_sites.npz")
    T = g["site_means"].shape[0]
    ssm = _gpu_ssm_from_golden(g, (), T)
    H = dev(np.broadcast_to(g["H"], (T,) + g["H"].shape).copy())
    sites = GaussianSitesNat(dev(g["site_means"] / g["site_covs"][..., 0]), dev(-0.5 / g["site_covs"]))
    kf = KalmanFilterWithSites(ssm, EmissionModel(H), sites)
    np.testing.assert_allclose(float(kf.log_likelihood()), g["log_lik_total"], rtol=1e-7)
    # the same through the fused entry point (time-invariant emission matrix declared: mfgm_kf_sites_elbo)
    kf2 = KalmanFilterWithSites(_gpu_ssm_from_golden(g, (), T), EmissionModel(H, constant_matrix=dev(g["H"])), sites)
    np.testing.assert_allclose(float(kf2.log_likelihood()), g["log_lik_total"], rtol=1e-7)
    post = kf.posterior_state_space_model()
    assert_close(host(post.marginal_means), g["smooth_means"])
    assert_close(host(post.marginal_covariances), g["smooth_covs"])


def test_kalman_filter_sparse_sites(amd, rng):
    """Sparse-site filter == oracle (kalman_filter.py:504-639; reference test_kalman_filter_with_sparse_sites.py)."""
    from oracle import np_kalman, np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.kalman_filter import GaussianSitesNat, KalmanFilterWithSparseSites
    T = 40
    t = np.linspace(0.0, 4.0, T)
    idx = np.sort(rng.choice(T, size=9, replace=False))
    y = rng.normal(size=(9, 1))
    nat1, nat2 = y / 0.3, -0.5 / 0.3 * np.ones((9, 1, 1))
    ok, gk = np_kernels.Matern32(0.9, 1.2), K.Matern32(0.9, 1.2)
    okf = np_kalman.KalmanFilterWithSparseSites(ok.state_space_model(t), ok.emission_matrix(t), np_kalman.GaussianSitesNat(nat1, nat2), T, idx, y)
    gkf = KalmanFilterWithSparseSites(gk.state_space_model(dev(t)), gk.generate_emission_model(dev(t)),
                                      GaussianSitesNat(dev(nat1), dev(nat2)), T, dev(idx), dev(y))
    np.testing.assert_allclose(float(gkf.log_likelihood()), okf.log_likelihood(), rtol=1e-8)


@pytest.mark.parametrize("kname", ["m12", "m52", "sum"])
def test_cvi_gaussian_process(amd, rng, kname):
    """KA7 on the GPU: CVIGaussianProcess one-step optimum == GPR log-likelihood, sites == (y, -1/2)/sigma^2, and the
    damped iteration against the oracle (reference tests/integration/models/test_variational_cvi.py:82-141)."""
    from oracle import np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess, GaussianProcessRegression
    mk = {"m12": (lambda m: m.Matern12(2.0, 2.25)), "m52": (lambda m: m.Matern52(0.8, 1.5)),
          "sum": (lambda m: m.Sum([m.Matern32(1.1, 0.7), m.Matern12(0.5, 1.2)]))}[kname]
    t = np.sort(rng.uniform(0, 4, size=8))
    y = np.cos(3 * t)[:, None] + 0.1 * rng.normal(size=(8, 1))
    noise = 1.0
    g = CVIGaussianProcess((dev(t), dev(y)), mk(K), Gaussian(noise), learning_rate=1.0)
    g.update_sites()
    np.testing.assert_allclose(host(g.sites.nat1), y / noise, rtol=1e-9)
    np.testing.assert_allclose(host(g.sites.nat2), -0.5 / noise * np.ones((8, 1, 1)), rtol=1e-9)
    gpr = GaussianProcessRegression((dev(t), dev(y)), mk(K), dev(np.sqrt(noise) * np.eye(1)))
    ref = np_models.gpr_log_likelihood(t, y, mk(np_kernels), noise)
    # Matern-5/2 process covariances Q = Pinf - A Pinf A^T lose ~8 digits to cancellation at the small random gaps used
    # here (in the reference as well), which bounds the agreement of any two evaluation orders: 5e-6 << the 1e-5 bound
    tol = 1e-8 if kname == "m12" else 5e-6
    np.testing.assert_allclose(float(gpr.log_likelihood()), ref, rtol=tol)
    np.testing.assert_allclose(float(g.elbo()), ref, rtol=tol)
    np.testing.assert_allclose(float(g.classic_elbo()), ref, rtol=max(tol, 1e-6))
    # damped updates follow the oracle
    g2 = CVIGaussianProcess((dev(t), dev(y)), mk(K), Gaussian(0.3), learning_rate=0.4)
    o2 = np_models.CVIGaussianProcess(t, y, mk(np_kernels), np_models.GaussianLik(0.3), learning_rate=0.4)
    for _ in range(3):
        g2.update_sites()
        o2.update_sites()
        np.testing.assert_allclose(float(g2.elbo()), o2.elbo(), rtol=max(tol, 1e-7))
        np.testing.assert_allclose(float(g2.classic_elbo()), o2.classic_elbo(), rtol=max(tol, 1e-6))


def test_cvi_step_graph_interleaved_with_eager_calls(amd, rng):
    """CVIGaussianProcess.step_graph(): replays of the captured `update_sites(); elbo()` interleaved with eager update_sites / elbo /
    classic_elbo / predict_f_at_data calls, and with a foreign factorisation on the same plan, give the ELBO sequence and sites of an
    all-eager run (the captured order is self-contained and every replay advances the host-side stamps the factor cache keys on)."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    T = 3000
    t = np.linspace(0.0, 30.0, T)
    y = np.sin(2 * t)[:, None] + 0.1 * rng.normal(size=(T, 1))
    mk = lambda: CVIGaussianProcess((dev(t), dev(y)), K.Matern52(0.5, 1.0), Gaussian(0.05), learning_rate=0.3)
    a, b = mk(), mk()
    step = b.step_graph()
    # the programme: "g" = one replay (a: update_sites + elbo), "u" = eager update_sites alone, "e" = eager elbo, "c" = classic_elbo,
    # "p" = predict_f_at_data, "x" = a foreign factorisation on the plan (the prior's marginals)
    got, want = [], []
    for op in "gugxgceupgxeg":
        for m, out, replay in ((a, want, False), (b, got, True)):
            if op == "g":
                if replay:
                    out.append(float(step()))
                else:
                    m.update_sites()
                    out.append(float(m.elbo()))
            elif op == "u":
                m.update_sites()
            elif op == "e":
                out.append(float(m.elbo()))
            elif op == "c":
                out.append(float(m.classic_elbo()))
            elif op == "p":
                out.append(float(m.predict_f_at_data()[0].sum()))
            else:
                pl = m.dist_p.plan
                nat = pl.ssm_to_naturals(m.dist_p.packed.A, m.dist_p.packed.off, m.dist_p.packed.chol, precision=False)
                f = pl.factor(nat["diag"], nat["sub"], nat["lin"], aD=-2.0, aS=-1.0)
                torch.cuda.synchronize()
    b.dist_p.plan.check_info()
    np.testing.assert_allclose(got, want, rtol=1e-10)
    np.testing.assert_allclose(host(b.sites.nat1), host(a.sites.nat1), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(host(b.sites.nat2), host(a.sites.nat2), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("d,B,T,kind", [(1, 1, 60, "dw"), (2, 2, 47, "dw"), (1, 2, 33, "ou"), (3, 1, 140, "dw"),
                                        (2, 2, 700, "ou"),      # 88 segments: more than one per lane of the Lagrange scan
                                        (6, 2, 150, "dw")])     # the bench's state dimension, ragged partition; oracle closed_form
def test_variational_markov_gp(amd, rng, d, B, T, kind):
    """VDP (vi_sde.py): forward pass, energy and gradients, Lagrange sweep, parameter / initial-state updates and ELBO
    against the oracle's restatement of the reference loop, per trajectory."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGP
    dt = 0.01
    qd = np.ones(d)
    osde = np_sde.OrnsteinUhlenbeckSDE(0.9, np.diag(qd)) if kind == "ou" else np_sde.DoubleWellSDE(np.diag(qd))
    gs = gsde.OrnsteinUhlenbeckSDE(0.9, torch.from_numpy(np.diag(qd))) if kind == "ou" else gsde.DoubleWellSDE(torch.from_numpy(np.diag(qd)))
    grid = np.arange(T) * dt
    idx = np.arange(5, T - 1, 9)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    cholR = 0.5 * np.eye(d)
    init = (np.zeros(d), 0.5 * np.eye(d))
    plan = amd.Plan(B, T, d, R0=8, Rup=3)
    g = VariationalMarkovGP((grid[idx], dev(y)), gs, grid, MultivariateGaussian(dev(cholR)), prior_initial_state=init, plan=plan)
    os_ = [np_models.VariationalMarkovGP(idx, y[b], osde, grid, np_models.MultivariateGaussianLik(cholR), *init, closed_form=d > 3)
           for b in range(B)]
    for it in range(5):
        mS = g._forward_packed()
        gm, gS = g._grad_E_sde(mS)
        g.update_lagrange(mS)
        g.update_param(mS, lr=0.05)
        if it > 1:
            g.update_initial_statistics(0.05)
        e = host(g.elbo_per_trajectory())
        psi, lam = host(plan.unpack(amd.FULL, g.psi_lagrange, T - 1)), host(plan.unpack(amd.VEC, g.lambda_lagrange, T - 1))
        A, bb = host(plan.unpack(amd.FULL, g.A, T - 1)), host(plan.unpack(amd.VEC, g.b, T - 1))
        for b, o in enumerate(os_):
            m, S = o.forward_pass()
            assert_close(host(plan.unpack(amd.VEC, mS[0]))[b], m)
            assert_close(host(plan.unpack(amd.SYM, mS[1]))[b], S)
            odm, odS = o._grad_E_sde(m, S)
            assert_close(host(gm)[b], odm)
            assert_close(host(gS)[b], odS)
            o.update_lagrange(m, S)
            assert_close(psi[b], o.psi)
            assert_close(lam[b], o.lam)
            o.update_param(m, S, 0.05)
            assert_close(A[b], o.A)
            assert_close(bb[b], o.b)
            if it > 1:
                o.update_initial_statistics(0.05)
            np.testing.assert_allclose(e[b], o.elbo(), rtol=1e-6, atol=1e-6)


def test_ssm_sample_log_pdf_and_udu(amd, rng):
    """StateSpaceModel.sample / log_pdf (state_space_model.py:298-324, 485-526) and upper_diagonal_lower
    (block_tri_diag.py:442-549; reference test_block_tri_diag.py:207-225: U D U^T recombines to the matrix)."""
    import torch
    from vidp_amd.block_tri_diag import SymmetricBlockTriDiagonal
    from vidp_amd.state_space_model import StateSpaceModel
    B, T, d = 2, 12, 3
    prm = random_ssm_params(rng, (B,), T, d)
    o = np_ssm.StateSpaceModel(*prm)
    g = StateSpaceModel(*[dev(p) for p in prm])
    x = o.sample((4,), rng)
    assert_close(host(g.log_pdf(dev(x))), o.log_pdf(x))
    gen = torch.Generator(device="cuda").manual_seed(3)
    xs = g.sample((3000,), generator=gen)
    assert tuple(xs.shape) == (3000, B, T, d)
    mu, cov = o.marginals
    np.testing.assert_allclose(host(xs.mean(0)), mu, atol=0.15)
    np.testing.assert_allclose(host(xs.var(0)), np.einsum("...ii->...i", cov), rtol=0.25, atol=0.05)
    assert tuple(g.sample((0,)).shape) == (0, B, T, d)
    diag, sub = random_dominant_btd(rng, (B,), 9, d)
    sym = SymmetricBlockTriDiagonal(dev(diag), dev(sub))
    ut, chol_d = sym.upper_diagonal_lower()
    Ut = host(ut.to_dense())
    cd = host(chol_d.block_diagonal)
    D = np_btd.to_dense(cd @ np.swapaxes(cd, -1, -2), None)
    np.testing.assert_allclose(np.swapaxes(Ut, -1, -2) @ D @ Ut, np_btd.to_dense(diag, sub), rtol=1e-6, atol=1e-8)
    ou, ocd = np_btd.upper_diagonal_lower(diag, sub)
    assert_close(host(ut.block_sub_diagonal), ou)
    assert_close(cd, ocd)


def test_trainers(amd, rng):
    """The trainer loops (cvi_dp_trainer.py:63-136, vi_markov_gp_trainer.py:50-135) on an OU problem: the CVI-DP trainer reaches
    the exact posterior (ELBO == log marginal likelihood of the Euler SSM) and both trainers' ELBOs end higher than they start."""
    import torch
    from oracle import np_btd
    from tests.test_oracle_models import ou_euler_ssm
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.trainers import CVISitesTrainer, VIMarkovGPTrainer
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    from vidp_amd.vi_sde import VariationalMarkovGP
    T, dt, decay = 80, 0.01, 1.2
    grid = np.arange(T) * dt
    idx = np.sort(rng.choice(np.arange(1, T - 1), size=10, replace=False))
    test_idx = np.array([i for i in range(3, T - 1, 7) if i not in set(idx)])
    y = rng.normal(size=(1, 10, 1))
    y_test = rng.normal(size=(1, len(test_idx), 1))
    lik = MultivariateGaussian(dev(0.3 * np.eye(1)))
    init = (np.zeros(1), np.eye(1) / (2 * decay))
    m = CVISitesSDE(gsde.OrnsteinUhlenbeckSDE(decay, torch.eye(1, dtype=torch.float64)), grid, (grid[idx], dev(y)), lik, prior_initial_state=init)
    tr = CVISitesTrainer(m, test_data=(grid[test_idx], dev(y_test)), girsanov_sites_lr=1.0, data_sites_lr=1.0, max_itr=3, max_itr_sites_optim=3)
    elbos, nlpds, rmses, _ = tr.optimize()
    ssm = ou_euler_ssm(T, dt, decay, 1.0)
    pd, ps = ssm.precision()
    K = np.linalg.inv(np_btd.to_dense(pd, ps))
    Kyy = K[np.ix_(idx, idx)] + 0.09 * np.eye(10)
    loglik = -0.5 * y[0, :, 0] @ np.linalg.solve(Kyy, y[0, :, 0]) - 0.5 * np.linalg.slogdet(Kyy)[1] - 5 * np.log(2 * np.pi)
    np.testing.assert_allclose(elbos[-1], loglik, rtol=1e-6, atol=1e-5)
    assert np.isfinite(nlpds[-1]) and np.isfinite(rmses[-1]) and elbos[-1] >= elbos[0]
    v = VariationalMarkovGP((grid[idx], dev(y)), gsde.OrnsteinUhlenbeckSDE(decay, torch.eye(1, dtype=torch.float64)), grid, lik,
                            prior_initial_state=init)
    tv = VIMarkovGPTrainer(v, test_data=(grid[test_idx], dev(y_test)), q_lr=0.05, x0_lr=0.05, max_itr=15, warmup_itr=2)
    ev, nv, rv, _ = tv.optimize()
    assert ev[-1] > ev[0] and np.isfinite(nv[-1])
    # VDP and CVI-DP approximate the same posterior: the VDP bound stays below the exact log marginal likelihood
    assert ev[-1] <= loglik + 1e-6


def test_trainer_metrics_and_batched_loop(amd, rng):
    """f-2: (i) NLPD / RMSE of the trainers against the oracle's restatement of exp_dp_utils.py:189-224 on the oracle model's own
    marginals, after the same site updates (CVI-DP, double well, d = 2; and the VDP trainer's metrics on its forward pass);
    (ii) CVISitesTrainer with one host synchronisation per 4 iterations (checkpoint + replay when a learning-rate rule fires inside a
    batch) against the plain per-iteration loop: the same ELBO / NLPD / RMSE sequences, the same learning rates and the same final
    state, on a problem whose learning rates are too large on purpose so that the decay rule fires."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.trainers import CVISitesTrainer, VIMarkovGPTrainer
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    from vidp_amd.vi_sde import VariationalMarkovGP
    B, T, d, dt = 2, 90, 2, 0.02
    grid = np.arange(T) * dt
    idx = np.arange(4, T - 1, 7)
    tidx = np.array([i for i in range(2, T - 1, 5) if i not in set(idx)])
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.2 * rng.normal(size=(B, len(idx), d))
    yt = np.sign(rng.normal(size=(B, len(tidx), d))) + 0.2 * rng.normal(size=(B, len(tidx), d))
    cholR = np.array([[0.3, 0.0], [0.1, 0.25]])
    init = (np.zeros(d), 0.5 * np.eye(d))
    mk = lambda: CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)),
                             prior_initial_state=init, plan=amd.Plan(B, T, d, R0=8, Rup=3))
    # (i) metrics against the oracle
    g = mk()
    os_ = [np_models.CVISitesSDE(np_sde.DoubleWellSDE(np.eye(d)), grid, idx, y[b], np_models.MultivariateGaussianLik(cholR), *init) for b in range(B)]
    tr = CVISitesTrainer(g, test_data=(grid[tidx], dev(yt)), data_sites_lr=0.5, girsanov_sites_lr=0.2)
    for m in [g] + os_:
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.2)
    _, nl, rm = tr._elbo_nlpd_rmse()
    marg = [o.dist_q.marginals for o in os_]
    want_nl = np.mean([np_models.calculate_nlpd(mu, S, cholR, grid, grid[tidx], yt[b]) for b, (mu, S) in enumerate(marg)])
    want_rm = np.sqrt(np.mean([np_models.calculate_rmse(mu, grid, grid[tidx], yt[b]) ** 2 for b, (mu, _) in enumerate(marg)]))
    np.testing.assert_allclose(nl, want_nl, rtol=1e-7)
    np.testing.assert_allclose(rm, want_rm, rtol=1e-7)
    v = VariationalMarkovGP((grid[idx], dev(y)), gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, MultivariateGaussian(dev(cholR)),
                            prior_initial_state=init, plan=amd.Plan(B, T, d, R0=8, Rup=3))
    ov = [np_models.VariationalMarkovGP(idx, y[b], np_sde.DoubleWellSDE(np.eye(d)), grid, np_models.MultivariateGaussianLik(cholR), *init)
          for b in range(B)]
    tv = VIMarkovGPTrainer(v, test_data=(grid[tidx], dev(yt)))
    mS = v._forward_packed()
    ev, nv, rv = tv._elbo_nlpd_rmse(mS)
    fw = [o.forward_pass() for o in ov]
    np.testing.assert_allclose(ev, sum(o.elbo(*f) for o, f in zip(ov, fw)), rtol=1e-8)
    np.testing.assert_allclose(nv, np.mean([np_models.calculate_nlpd(m_, S_, cholR, grid, grid[tidx], yt[b]) for b, (m_, S_) in enumerate(fw)]), rtol=1e-7)
    np.testing.assert_allclose(rv, np.sqrt(np.mean([np_models.calculate_rmse(m_, grid, grid[tidx], yt[b]) ** 2 for b, (m_, _) in enumerate(fw)])), rtol=1e-7)
    # (ii) batched loop == plain loop; learning rates large enough for the ELBO to drop at some iteration
    def run(k, lr_d, lr_g, tol):
        m = mk()
        t = CVISitesTrainer(m, test_data=(grid[tidx], dev(yt)), data_sites_lr=lr_d, girsanov_sites_lr=lr_g, max_itr_sites_optim=14,
                            optim_tol=tol, sync_every=k)
        e, n, r = t._optimize_sites_under_stable_prior()
        return (np.array(e), np.array(n), np.array(r), t.data_sites_lr, t.girsanov_sites_lr, host(m.plan.unpack(amd.VEC, m.full_sites().lin)))

    def same(a, b):
        assert len(a[0]) == len(b[0]) and (a[3], a[4]) == (b[3], b[4])
        for x, y_ in zip(a[:3], b[:3]):
            np.testing.assert_allclose(y_, x, rtol=1e-12)
        assert_close(b[5], a[5], rtol=1e-12)

    # the decay rule: over-relaxed data sites (|1 - lr| < 1: they still converge, but alternating around the fixed point) make the plain
    # loop's ELBO drop at some iteration without driving the posterior away
    plain = None
    for lr_d, lr_g in ((1.8, 0.3), (1.9, 0.3), (1.7, 0.6), (1.95, 0.2)):
        try:
            cand = run(1, lr_d, lr_g, 1e-9)
        except ArithmeticError:
            continue
        if cand[3] < lr_d and np.isfinite(cand[0]).all():
            plain = (lr_d, lr_g, cand)
            break
    assert plain is not None, "no learning rate made the decay rule fire"
    same(plain[2], run(4, plain[0], plain[1], 1e-9))
    same(plain[2], run(3, plain[0], plain[1], 1e-9))
    # the convergence rule firing inside a batch
    conv = run(1, 0.5, 0.2, 0.5)
    assert 2 < len(conv[0]) < 14
    same(conv, run(4, 0.5, 0.2, 0.5))


def test_ssm_natgrad_one_step_optimum(amd, rng):
    """KA9 (reference tests/integration/test_ssm_natgrad.py:46-65): one natural-gradient step with gamma = 1 and a Gaussian
    likelihood makes the variational ELBO equal to the GPR log-likelihood (atol 1e-5, rtol 1e-6), from any initial q."""
    from oracle import np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.ssm_natgrad import GaussMarkovELBO, SSMNaturalGradient
    from vidp_amd.state_space_model import StateSpaceModel
    mk = lambda m: m.Sum([m.Matern52(0.9, 1.3), m.Matern32(1.4, 0.6)])
    t = np.sort(rng.uniform(0, 5, size=10))
    y = np.sin(2 * t)[:, None] + 0.1 * rng.normal(size=(10, 1))
    noise = 0.5
    gk = mk(K)
    p = gk.state_space_model(dev(t))
    plan = p.plan
    q = StateSpaceModel(*[dev(a) for a in random_ssm_params(rng, (), 10, 5)], plan=plan)
    loss = GaussMarkovELBO(p, gk.generate_emission_model(dev(t)), Gaussian(noise), dev(y))
    before = float(loss.elbo(q))
    SSMNaturalGradient(gamma=1.0, momentum=False).minimize(loss, q)
    ref = np_models.gpr_log_likelihood(t, y, mk(np_kernels), noise)
    np.testing.assert_allclose(float(loss.elbo(q)), ref, rtol=1e-6, atol=1e-5)
    assert float(loss.elbo(q)) > before
    # a damped step moves towards, not onto, the optimum
    q2 = StateSpaceModel(*[dev(a) for a in random_ssm_params(rng, (), 10, 5)], plan=plan)
    e0 = float(loss.elbo(q2))
    SSMNaturalGradient(gamma=0.3, momentum=False).minimize(loss, q2)
    e1 = float(loss.elbo(q2))
    assert e0 < e1 < ref + 1e-6
    # (plain closures go through the tape route: test_ssm_natgrad_tape_route)


def test_ssm_natgrad_momentum(amd, rng):
    """The Adam-like variant (ssm_natgrad.py:177-208, the reference's default; no reference test exists): the Fisher norm of the
    natural gradient against a dense evaluation of g^T (d eta / d theta) g, and the first update against the documented formulas."""
    from vidp_amd import kernels as K, ssm_gaussian_transformations as tr
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.ssm_natgrad import GaussMarkovELBO, SSMNaturalGradient
    from vidp_amd.state_space_model import StateSpaceModel
    T, d = 7, 3
    gk = K.Sum([K.Matern32(1.4, 0.6), K.Matern12(0.7, 1.1)])
    t = np.sort(rng.uniform(0, 5, size=T))
    y = np.sin(2 * t)[:, None] + 0.1 * rng.normal(size=(T, 1))
    p = gk.state_space_model(dev(t))
    q = StateSpaceModel(*[dev(a) for a in random_ssm_params(rng, (), T, d)], plan=p.plan)
    loss = GaussMarkovELBO(p, gk.generate_emission_model(dev(t)), Gaussian(0.5), dev(y))
    pl = q.plan
    (gl, gd, gs), nq = loss.grad_wrt_expectations(q)
    norm = SSMNaturalGradient.natgrad_norm(pl, nq, (gl, gd, gs))
    # dense reference: P = blocktridiag(-2 theta_diag, -theta_sub), mu = P^{-1} theta_lin; direction v = g
    th = [host(x)[0] for x in (pl.unpack(amd.VEC, nq["lin"]), pl.unpack(amd.SYM, nq["diag"]), pl.unpack(amd.FULL, nq["sub"], T - 1))]
    v = [host(x)[0] for x in (pl.unpack(amd.VEC, gl), pl.unpack(amd.SYM, gd), pl.unpack(amd.FULL, gs, T - 1))]
    def dense(diag, sub):
        M = np.zeros((T * d, T * d))
        for k in range(T):
            M[k * d:(k + 1) * d, k * d:(k + 1) * d] = -2.0 * diag[k]
        for k in range(T - 1):
            M[(k + 1) * d:(k + 2) * d, k * d:(k + 1) * d] = -sub[k]
            M[k * d:(k + 1) * d, (k + 1) * d:(k + 2) * d] = -sub[k].T
        return M
    P, dP = dense(th[1], th[2]), dense(v[1], v[2])
    S = np.linalg.inv(P)
    mu = S @ th[0].reshape(-1)
    dmu = S @ (v[0].reshape(-1) - dP @ mu)
    dE = -S @ dP @ S + np.outer(dmu, mu) + np.outer(mu, dmu)
    ref = v[0].reshape(-1) @ dmu
    for k in range(T):
        ref += np.sum(v[1][k] * dE[k * d:(k + 1) * d, k * d:(k + 1) * d])
    for k in range(T - 1):
        ref += 2.0 * np.sum(v[2][k] * dE[(k + 1) * d:(k + 2) * d, k * d:(k + 1) * d])
    assert ref > 0
    np.testing.assert_allclose(norm, ref, rtol=1e-6)
    # first step: m = (1-b1) g, v = (1-b2) norm, lr = gamma sqrt(1-b2)/(1-b1)
    opt = SSMNaturalGradient(gamma=0.2, beta1=0.9, beta2=0.99, epsilon=1e-8)      # momentum is the default, as in the reference
    e0 = float(loss.elbo(q))
    opt.minimize(loss, q)
    step = 0.2 * np.sqrt(1 - 0.99) / (1 - 0.9) / (np.sqrt((1 - 0.99) * ref) + 1e-8) * (1 - 0.9)
    want = [a - step * b for a, b in zip(th, v)]
    got = tr.ssm_to_naturals(q)
    for a, b in zip(got, want):
        assert_close(host(a), b, rtol=1e-5)
    assert float(loss.elbo(q)) > e0
    opt.minimize(loss, q)           # second step runs with the moving averages
    assert np.isfinite(float(loss.elbo(q)))


@pytest.mark.parametrize("kname", ["m12", "m32sum"])
def test_sparse_cvi_and_posterior(amd, rng, kname):
    """KA8 on the GPU: SparseCVIGaussianProcess with z = x (one-step optimum == GPR log-likelihood, optimal sites), with z != x
    against the oracle, and ConditionalProcess.predict_f at new time points (posterior.py / conditionals.py)."""
    from oracle import np_conditionals as npc, np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    mk = {"m12": (lambda m: m.Matern12(0.3, 1.5)), "m32sum": (lambda m: m.Sum([m.Matern32(0.4, 1.0), m.Matern12(0.7, 0.5)]))}[kname]
    N = 12
    t = np.linspace(0, 1, N)
    y = (np.cos(20 * t) + rng.normal(size=N)).reshape(-1, 1)
    g = SparseCVIGaussianProcess(mk(K), dev(t), Gaussian(1.0), learning_rate=1.0)
    g.update_sites((dev(t), dev(y)))
    sd = mk(K).state_dim
    ref = np_models.gpr_log_likelihood(t, y, mk(np_kernels), 1.0)
    np.testing.assert_allclose(float(g.classic_elbo((dev(t), dev(y)))), ref, rtol=1e-6)
    if kname == "m12":
        np.testing.assert_allclose(host(g.nat1)[:-1, sd:], y, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(host(g.nat2)[:-1, sd:, sd:], -0.5 * np.ones((N, 1, 1)), rtol=1e-8)
    # inducing points different from the data, damped updates: follow the oracle
    z = np.linspace(-0.1, 1.1, 7)
    g2 = SparseCVIGaussianProcess(mk(K), dev(z), Gaussian(0.5), learning_rate=0.6)
    o2 = npc.SparseCVIGaussianProcess(mk(np_kernels), z, np_models.GaussianLik(0.5), learning_rate=0.6)
    prev = -np.inf
    for _ in range(3):
        g2.update_sites((dev(t), dev(y)))
        o2.update_sites(t, y)
        e = float(g2.classic_elbo((dev(t), dev(y))))
        np.testing.assert_allclose(e, o2.classic_elbo(t, y), rtol=1e-6)
        assert e > prev - 1e-9
        prev = e
    tn = np.sort(rng.uniform(-0.3, 1.3, size=9))
    mu, var = g2.posterior.predict_f(dev(tn))
    omu, ovar = npc.predict_f(o2.dist_q, mk(np_kernels), z, tn)
    assert_close(host(mu), omu)
    assert_close(host(var), ovar)


def test_exp_io_checkpoints(amd, rng, tmp_path):
    """On-disk formats of the reference's experiments: data .npz schema (exp_dp_utils.py:108-125), cvi_model.npz /
    posteriors.npz (cvi_dp.py:140-149), vi_gp_model.npz (vi_markov_gp.py:175-178) and the CVI-DP -> VDP warm start
    (vi_markov_gp.py:89-115): key names and shapes as the reference writes them, and save -> load reproduces the model."""
    import torch
    from vidp_amd import exp_io, sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    from vidp_amd.vi_sde import VariationalMarkovGP
    T, dt, d = 70, 0.01, 2
    grid = np.arange(T) * dt
    idx = np.arange(4, T - 1, 6)
    y = np.sign(rng.normal(size=(1, len(idx), d))) + 0.1 * rng.normal(size=(1, len(idx), d))
    path = str(tmp_path / "data.npz")
    exp_io.save_exp_data(path, Q=np.eye(d), x0=np.ones(d), sigma=0.3, latent_process=rng.normal(size=(T, d)), observation_grid=grid[idx],
                         observations=y[0], test_grid=grid[[3, 9]], test_observations=y[0, :2], time_grid=grid)
    Q, x0, noise, latent, obs, tg, test = exp_io.load_exp_data(path)
    assert noise.shape == (1, 1) and tuple(obs[1].shape) == (len(idx), d) and obs[0].is_cuda and tuple(tg.shape) == (T,)
    np.testing.assert_array_equal(host(obs[1]), y[0])
    lik = MultivariateGaussian(dev(noise.item() * np.eye(d)))
    init = (np.zeros(d), np.eye(d))
    mk = lambda: CVISitesSDE(gsde.DoubleWellSDE(q=torch.eye(d, dtype=torch.float64)), grid, (obs[0], obs[1][None]), lik, prior_initial_state=init)
    m = mk()
    for _ in range(3):
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.2)
    out = str(tmp_path / "run")
    exp_io.save_cvi_model(out, m)
    z = np.load(out + "/cvi_model.npz")
    assert sorted(z.files) == sorted(["data_sites_nat1", "data_sites_nat2", "girsanov_sites_nat1", "girsanov_sites_nat2_diag",
                                      "girsanov_sites_nat2_subdiag"])
    assert z["data_sites_nat1"].shape == (len(idx), d) and z["girsanov_sites_nat2_subdiag"].shape == (T - 1, d, d)
    post = np.load(out + "/posteriors.npz")
    assert post["cvi_m"].shape == (T, d) and post["cvi_S"].shape == (T, d, d) and post["time_grid"].shape == (T,)
    m2 = exp_io.load_cvi_model(out, mk())
    np.testing.assert_allclose(host(m2.classic_elbo_per_trajectory()), host(m.classic_elbo_per_trajectory()), rtol=1e-10)
    mu2, S2 = m2.dist_q.marginals
    assert_close(host(mu2).reshape(T, d), post["cvi_m"], rtol=1e-9)
    assert_close(host(S2).reshape(T, d, d), post["cvi_S"], rtol=1e-9)
    # VDP: warm start from the CVI posterior, checkpoint round trip
    mkv = lambda: VariationalMarkovGP((obs[0], obs[1][None]), gsde.DoubleWellSDE(q=torch.eye(d, dtype=torch.float64)), grid, lik,
                                      prior_initial_state=init)
    v = exp_io.warm_start_vdp_from_cvi(mkv(), m)
    ssm = m.dist_q
    A_ref = -(host(ssm.state_transitions).reshape(T - 1, d, d) - np.eye(d)) / dt
    assert_close(host(v.plan.unpack(amd.FULL, v.A, T - 1))[0], A_ref, rtol=1e-12)
    assert_close(host(v.plan.unpack(amd.VEC, v.b))[0, :T - 1], host(ssm.state_offsets).reshape(T - 1, d) / dt, rtol=1e-12)
    mS = v._forward_packed()
    v.update_lagrange(mS)
    v.update_param(mS, lr=0.05)
    exp_io.save_vi_gp_model(out, v)
    zv = np.load(out + "/vi_gp_model.npz")
    assert sorted(zv.files) == sorted(["A", "b", "lambda_lagrange", "psi_lagrange", "x0_m", "x0_S"])
    assert zv["A"].shape == (T - 1, d, d) and zv["lambda_lagrange"].shape == (T - 1, d) and zv["x0_S"].shape == (d, d)
    v2 = exp_io.load_vi_gp_model(out, mkv())
    np.testing.assert_allclose(host(v2.elbo_per_trajectory()), host(v.elbo_per_trajectory()), rtol=1e-10)
    with pytest.raises(ValueError):
        exp_io.load_vi_gp_model(out, VariationalMarkovGP((obs[0][:3], obs[1][None, :3]), gsde.DoubleWellSDE(q=torch.eye(d, dtype=torch.float64)),
                                                         grid[:40], lik, prior_initial_state=init))


def test_prior_parameter_gradients_and_learning(amd, rng):
    """Prior learning (variational_cvi_sde.py:495-518, cvi_dp_trainer.py:207-250).  grad_KL_wrt_prior_params against
    finite differences of the oracle's KL (closed form and, at d = 1, the reference's 20-point quadrature route) at the GPU
    posterior; grad_VE_wrt_prior_params against finite differences over freshly built models carrying the same sites; and the
    trainer's learning loop moves a mis-specified OU decay towards the data-generating one while the ELBO rises."""
    import torch
    from oracle import np_sde
    from vidp_amd import exp_io, sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.trainers import CVISitesTrainer
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    T, dt, d = 60, 0.01, 1
    grid = np.arange(T) * dt
    idx = np.arange(4, T - 1, 5)
    y = np.sign(rng.normal(size=(1, len(idx), d))) + 0.1 * rng.normal(size=(1, len(idx), d))
    lik = MultivariateGaussian(dev(0.3 * np.eye(d)))
    init = (np.zeros(d), np.eye(d))
    sde = gsde.DoubleWellSDE(q=torch.eye(d, dtype=torch.float64), scale_trainable=True, c_trainable=True, scale=3.0, c=0.8)
    assert sde.trainable_variables == ["scale", "c"]
    m = CVISitesSDE(sde, grid, (grid[idx], dev(y)), lik, prior_initial_state=init)
    for _ in range(3):
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.2)
    g = m.grad_KL_wrt_prior_params()
    pm, pS, pC = m.dist_q_marginals_packed          # property: packed (mu, Sigma_tt, Sigma_{t+1,t})
    mu, Sig, Sub = [host(x)[0] for x in (m.plan.unpack(amd.VEC, pm), m.plan.unpack(amd.SYM, pS), m.plan.unpack(amd.FULL, pC, T - 1))]
    q = m.dist_q
    qA, qb, qcQ = host(q.state_transitions)[0], host(q.state_offsets)[0], host(q.cholesky_process_covariances)[0]

    def kl_closed(scale, c):
        o = np_sde.DoubleWellSDE(np.eye(d), scale, c)
        al, be = o.cubic(dt)
        return np_sde.sde_ssm_kl_closed_form(mu, Sig, Sub, al, be, np.ones(d), dt, *init)[0]

    def kl_quad(scale, c):
        o = np_sde.DoubleWellSDE(np.eye(d), scale, c)
        Qq = qcQ @ np.swapaxes(qcQ, -1, -2)
        f_q = lambda x: (qA[None] @ x[..., None])[..., 0] + qb[None]
        f_p = lambda x: x + dt * o.drift(x)
        return np_sde.ssm_kl_along_gaussian_path(f_q, f_p, Qq, np.broadcast_to(dt * np.eye(d), Qq.shape), mu, Sig)

    for kl in (kl_closed, kl_quad):
        h = 1e-5
        fd = [(kl(3.0 + h, 0.8) - kl(3.0 - h, 0.8)) / (2 * h), (kl(3.0, 0.8 + h) - kl(3.0, 0.8 - h)) / (2 * h)]
        np.testing.assert_allclose(g, fd, rtol=2e-5, atol=1e-7)

    # VE gradient: OU prior (linearisation independent of the path); reference value from fresh models carrying the same sites
    import tempfile
    ou = gsde.OrnsteinUhlenbeckSDE(0.7, torch.eye(d, dtype=torch.float64), trainable=True)
    mo = CVISitesSDE(ou, grid, (grid[idx], dev(y)), lik, prior_initial_state=init, stabilize_ssm=False)
    for _ in range(2):
        mo.update_data_sites(0.5)
        mo.update_girsanov_sites(0.3)
    gve = mo.grad_VE_wrt_prior_params()
    with tempfile.TemporaryDirectory() as tmp:
        exp_io.save_cvi_model(tmp, mo)

        def neg_ve(decay):
            mm = CVISitesSDE(gsde.OrnsteinUhlenbeckSDE(decay, torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), lik,
                             prior_initial_state=init, stabilize_ssm=False)
            exp_io.load_cvi_model(tmp, mm)
            return -float(mm.variational_expectation().sum())
        h = 1e-4
        np.testing.assert_allclose(gve, [(neg_ve(0.7 + h) - neg_ve(0.7 - h)) / (2 * h)], rtol=1e-5)
    # the exact chain rule (one Fisher-vector product for all parameters) against the round-2 evaluation (two re-linearised posterior
    # refreshes per parameter): double-well prior with both parameters trainable, d = 2, two trajectories, stabilised (clipped) prior
    d2 = 2
    y2 = np.sign(rng.normal(size=(2, len(idx), d2))) + 0.1 * rng.normal(size=(2, len(idx), d2))

    def dw_model():
        sd = gsde.DoubleWellSDE(q=torch.eye(d2, dtype=torch.float64), scale_trainable=True, c_trainable=True, scale=3.0, c=0.8)
        mm = CVISitesSDE(sd, grid, (grid[idx], dev(y2)), MultivariateGaussian(dev(0.3 * np.eye(d2))), prior_initial_state=(np.zeros(d2), np.eye(d2)))
        for _ in range(3):
            mm.update_data_sites(0.5)
            mm.update_girsanov_sites(0.2)
        return mm
    exact = dw_model().grad_VE_wrt_prior_params()
    fd = dw_model().grad_VE_wrt_prior_params(finite_difference=True)
    assert len(exact) == 2 and max(abs(v) for v in exact) > 1e-3
    np.testing.assert_allclose(exact, fd, rtol=2e-5, atol=1e-8)

    # learning loop: data from an OU process with decay 2, prior initialised at decay 0.3
    Tl, decay_true = 400, 2.0
    gridl = np.arange(Tl) * dt
    x = np.zeros(Tl)
    for k in range(1, Tl):
        x[k] = x[k - 1] - dt * decay_true * x[k - 1] + np.sqrt(dt) * rng.normal()
    il = np.arange(2, Tl - 1, 3)
    yl = (x[il] + 0.05 * rng.normal(size=len(il))).reshape(1, -1, 1)
    oul = gsde.OrnsteinUhlenbeckSDE(0.3, torch.eye(1, dtype=torch.float64), trainable=True)
    ml = CVISitesSDE(oul, gridl, (gridl[il], dev(yl)), MultivariateGaussian(dev(0.05 * np.eye(1))),
                     prior_initial_state=(np.zeros(1), np.eye(1) / 0.6), stabilize_ssm=False)
    tr = CVISitesTrainer(ml, girsanov_sites_lr=1.0, data_sites_lr=1.0, max_itr=3, max_itr_sites_optim=3, learn_prior_sde=True,
                         prior_sde_lr=0.2, learning_max_itr=15, learning_tol=1e-3)
    elbos, _, _, params = tr.optimize()
    assert len(params[0]) > 3 and params[0][0] == 0.3
    assert params[0][-1] > 0.6                    # moved towards the data-generating decay
    assert elbos[-1] > elbos[1]


def test_vdp_prior_gradient_and_learning(amd, rng):
    """VariationalMarkovGP.grad_prior_sde_params (vi_sde.py:457-470) against finite differences of the oracle's E_sde (closed
    form; at d = 1 also the reference's quadrature) on the same (m[1:], S[1:]) path, and the trainer's prior-learning loop
    (vi_markov_gp_trainer.py:163-201) raising the bound for a mis-specified OU decay."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.trainers import VIMarkovGPTrainer
    from vidp_amd.vi_sde import VariationalMarkovGP
    for d in (1, 2):
        T, dt = 50, 0.01
        grid = np.arange(T) * dt
        idx = np.arange(4, T - 1, 6)
        y = np.sign(rng.normal(size=(1, len(idx), d))) + 0.1 * rng.normal(size=(1, len(idx), d))
        sde = gsde.DoubleWellSDE(q=torch.eye(d, dtype=torch.float64), scale_trainable=True, c_trainable=True, scale=3.0, c=0.8)
        v = VariationalMarkovGP((grid[idx], dev(y)), sde, grid, MultivariateGaussian(dev(0.4 * np.eye(d))),
                                prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)))
        for _ in range(4):
            mS = v._forward_packed()
            v.update_lagrange(mS)
            v.update_param(mS, lr=0.05)
        g = v.grad_prior_sde_params()
        m, S = [host(x)[0][1:] for x in v.forward_pass]
        A = host(v.plan.unpack(amd.FULL, v.A, T - 1))[0]
        b = host(v.plan.unpack(amd.VEC, v.b))[0, :T - 1]

        def e_closed(scale, c):
            return np_sde.e_sde_closed_form(scale * c, scale, np.ones(d), -A, b, m, S, dt, want_grads=False)
        fns = [e_closed]
        if d == 1:
            def e_quad(scale, c):
                o = np_sde.DoubleWellSDE(np.eye(d), scale, c)
                return np_sde.squared_drift_difference_along_gaussian_path(o, -A, b, m, S, dt)
            fns.append(e_quad)
        for fn in fns:
            h = 1e-5
            fd = [(fn(3.0 + h, 0.8) - fn(3.0 - h, 0.8)) / (2 * h), (fn(3.0, 0.8 + h) - fn(3.0, 0.8 - h)) / (2 * h)]
            np.testing.assert_allclose(g, fd, rtol=2e-5, atol=1e-7)
    # gradient of KL[q(x0) || p(x0)] with respect to the prior's (loc, scale): finite differences of the oracle's Gaussian KL
    g_loc, g_scale = v.grad_initial_state()
    q0m, q0S = host(v.q0_mu)[0], host(v.q0_chol @ v.q0_chol.transpose(-1, -2))[0]
    Lp = np.linalg.cholesky(v.p0_cov)
    kl0 = lambda loc, L: np_sde.gauss_kl(q0m, q0S, loc, L @ L.T)
    h = 1e-6
    for i in range(d):
        e = np.zeros(d); e[i] = h
        np.testing.assert_allclose(host(g_loc)[i], (kl0(v.p0_mu + e, Lp) - kl0(v.p0_mu - e, Lp)) / (2 * h), rtol=1e-5, atol=1e-8)
        for j in range(i + 1):
            E = np.zeros((d, d)); E[i, j] = h
            np.testing.assert_allclose(host(g_scale)[i, j], (kl0(v.p0_mu, Lp + E) - kl0(v.p0_mu, Lp - E)) / (2 * h), rtol=1e-5, atol=1e-8)
    # learning: OU data with decay 2, prior initialised at 0.3 (gentle VDP step sizes: the fixed-point iteration diverges otherwise)
    T, dt = 120, 0.01
    grid = np.arange(T) * dt
    x = np.zeros(T)
    for k in range(1, T):
        x[k] = x[k - 1] - dt * 2.0 * x[k - 1] + np.sqrt(dt) * rng.normal()
    il = np.arange(2, T - 1, 4)
    yl = (x[il] + 0.3 * rng.normal(size=len(il))).reshape(1, -1, 1)
    ou = gsde.OrnsteinUhlenbeckSDE(0.3, torch.eye(1, dtype=torch.float64), trainable=True)
    vm = VariationalMarkovGP((grid[il], dev(yl)), ou, grid, MultivariateGaussian(dev(0.3 * np.eye(1))),
                             prior_initial_state=(np.zeros(1), np.eye(1) / 0.6))
    tr = VIMarkovGPTrainer(vm, q_lr=0.05, x0_lr=0.05, max_itr=15, warmup_itr=2, learn_prior_sde=True, prior_sde_lr=0.05,
                           learning_max_itr=8, learning_tol=1e-5, optimize_prior_initial_state=True)
    e_inf, _, _ = tr.perform_inference()
    assert np.isfinite(e_inf[-1]) and e_inf[-1] > e_inf[0]
    e_learn, _, _ = tr.optimize_prior_sde()
    assert np.all(np.isfinite(e_learn))
    assert tr.prior_params[0][0] == 0.3 and tr.prior_params[0][-1] > 0.3 + 0.2      # Adam moved the decay up, towards 2
    assert e_learn[-1] > e_inf[-1]                                                   # and the bound with it


def _theta_sdes(kind, d, qd):
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    q_np, q_t = np.diag(qd), torch.from_numpy(np.diag(qd))
    if kind == "benes":
        return np_sde.BenesSDE(1.3, q_np), gsde.BenesSDE(1.3, q_t)
    if kind == "sine":
        return np_sde.SineDiffusionSDE(0.4, q_np), gsde.SineDiffusionSDE(0.4, q_t)
    return np_sde.SqrtDiffusionSDE(1.5, q_np), gsde.SqrtDiffusionSDE(1.5, q_t)


@pytest.mark.parametrize("d,kind", [(1, "benes"), (1, "sine"), (2, "benes"), (2, "sine"), (1, "sqrt")])
def test_sde_kl_kernel_quadrature_drifts(amd, rng, d, kind):
    """Non-polynomial drifts (BenesSDE, SineDiffusionSDE, SqrtDiffusionSDE; sde.py:227-356): KL[q || p_SDE] (full-block and
    moment-array kernels), its gradient with respect to the expectation parameters and the linearisation, with the
    reference's Gauss-Hermite rules inside the kernels, against the oracle's restatement of the reference quadrature
    (sde_utils.py:262-359, 119-179; central differences stand in for the GradientTape)."""
    from oracle import np_sde
    B, T, dt = 2, 6, 0.05
    qd = 0.5 + rng.random(d)
    osde, gs = _theta_sdes(kind, d, qd)
    prm = random_ssm_params(rng, (B,), T, d, scale_A=0.8)
    # marginal standard deviations around 0.4: there the 20-point rule integrates tanh to ~1e-12, so the per-dimension
    # (Stein) form used by the kernels and the reference's quadrature of the squared residual are the same number
    prm = (prm[0], 0.4 * prm[1], prm[2], prm[3], 0.4 * prm[4])
    if kind == "sqrt":      # keep the path away from the kink at 0 (f' is singular there, in the reference too)
        prm = (prm[0] + 4.0, 0.5 * prm[1], 0.02 * prm[2] + 0.99 * np.eye(d), 0.02 * prm[3] + 0.05, 0.5 * prm[4])
    init_mu, init_cov = 0.1 * rng.normal(size=d), 0.7 * np.eye(d) + 0.1 * np.ones((d, d))
    plan = amd.Plan(B, T, d, R0=3, Rup=2)
    mus, covs, subs = [], [], []
    for b in range(B):
        q = np_ssm.StateSpaceModel(*[p[b] for p in prm])
        mu, cov = q.marginals
        mus.append(mu); covs.append(cov); subs.append(q.subsequent_covariances(cov))
    mu, cov, sub = np.stack(mus), np.stack(covs), np.stack(subs)
    pm, pc, ps = plan.pack(amd.VEC, dev(mu)), plan.pack(amd.SYM, dev(cov)), plan.pack(amd.FULL, dev(sub))
    cprm = gs.params(dt, init_mu, init_cov)
    grads = (plan.empty(amd.VEC), plan.empty(amd.SYM), plan.empty(amd.FULL))
    kl0 = host(plan.sde_kl(cprm, pm, pc, ps, mode=0))
    kl1 = host(plan.sde_kl(cprm, pm, pc, ps, mode=1, grads=grads))
    plan.check_info()
    g1, gd, gsub = host(plan.unpack(amd.VEC, grads[0])), host(plan.unpack(amd.SYM, grads[1])), host(plan.unpack(amd.FULL, grads[2], T - 1))
    A, off, chol = plan.linearize_cubic(gs.params(dt, init_mu, init_cov, clip=None), pm, pc)
    Ag, offg = host(plan.unpack(amd.FULL, A, T - 1)), host(plan.unpack(amd.VEC, off))
    for b in range(B):
        eta_d = cov[b] + mu[b][:, :, None] * mu[b][:, None, :]
        eta_s = sub[b] + mu[b][1:, :, None] * mu[b][:-1, None, :]
        kl = np_sde.sde_ssm_kl_from_expectations(mu[b], eta_d, eta_s, osde, dt, init_mu, init_cov)
        np.testing.assert_allclose(kl0[b], kl, rtol=1e-8)
        np.testing.assert_allclose(kl1[b], kl, rtol=1e-8)
        o1, od, os_ = np_sde.sde_ssm_kl_grads_fd(mu[b], eta_d, eta_s, osde, dt, init_mu, init_cov)
        assert_close(g1[b], o1, rtol=2e-5, scale_atol=1e-7)
        assert_close(gd[b], od, rtol=2e-5, scale_atol=1e-7)
        assert_close(gsub[b], os_, rtol=2e-5, scale_atol=1e-7)
        # the model linearises transition k around the posterior marginal of state k + 1 (variational_cvi_sde.py:408-432)
        lin = np_sde.linearize_sde(osde, np.arange(T) * dt, mu[b][1:], cov[b][1:], init_mu, init_cov)
        # d > 1: the reference's tensor-product 10-point rule and the per-dimension rule differ by the rule's own error
        assert_close(Ag[b], lin.A, rtol=1e-9 if d == 1 else 2e-6)
        assert_close(offg[b][1:], lin.b, rtol=1e-9 if d == 1 else 2e-6, scale_atol=1e-8 if d == 1 else 1e-6)


@pytest.mark.parametrize("kind", ["benes", "sine"])
def test_cvi_sites_sde_quadrature_drifts(amd, rng, kind):
    """CVI-DP with a non-polynomial prior drift (the lean moment-array path with Gauss-Hermite expectations) against the
    oracle model whose Girsanov gradient is the finite-differenced reference quadrature."""
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    d, B, T, dt = 1, 1, 12, 0.05
    osde, gs = _theta_sdes(kind, d, np.ones(d))
    grid = np.arange(T) * dt
    idx = np.array([3, 7, 10])
    y = np.sign(rng.normal(size=(B, 3, d))) + 0.2 * rng.normal(size=(B, 3, d))
    cholR = 0.3 * np.eye(d)
    init = (np.zeros(d), 0.5 * np.eye(d))
    g = CVISitesSDE(gs, grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)), prior_initial_state=init)
    o = np_models.CVISitesSDE(osde, grid, idx, y[0], np_models.MultivariateGaussianLik(cholR), *init)
    assert_close(host(g.dist_p.state_transitions)[0], o.dist_p.A)
    for lr_d, lr_g in ((0.5, 0.2), (0.3, 0.1)):
        g.update_data_sites(lr_d)
        g.update_girsanov_sites(lr_g)
        o.update_data_sites(lr_d)
        o.update_girsanov_sites(lr_g)
        np.testing.assert_allclose(host(g.classic_elbo_per_trajectory())[0], o.classic_elbo(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(host(g.KL_q_p()), host(g.KL_q_p_full()), rtol=1e-9)
    g.relinearize()
    o.relinearize()
    np.testing.assert_allclose(host(g.classic_elbo_per_trajectory())[0], o.classic_elbo(), rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("kind", ["vanderpol", "vanderpol_fullq", "mlp", "benes", "sine"])
def test_variational_markov_gp_quadrature_drifts(amd, rng, kind):
    """VDP with the drifts the closed-form kernels do not cover and with a full diffusion matrix (the reference's VariationalMarkovGP
    takes any SDE: vi_sde.py:377-414, 422-434): VariationalMarkovGPQuadrature on the HIP quadrature kernels against the oracle's
    restatement of the reference loop -- forward pass, E_sde and its gradients (oracle: exact for the polynomial drift, fourth-order quotients of its quadrature for the network), the
    Lagrange sweep, parameter / initial-state updates and the ELBO over a few iterations; and the drift-parameter gradient against a
    difference quotient of E_sde."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGPQuadrature
    T, dt = 30, 0.02
    grid = np.arange(T) * dt
    if kind.startswith("vanderpol"):
        d = 2
        q = 0.5 * np.eye(2) if kind == "vanderpol" else np.array([[0.5, 0.12], [0.12, 0.4]])
        o_sde, g_sde = np_sde.VanderPolSDE(1.3, 0.9, q), gsde.VanderPolOscillatorSDE(1.3, 0.9, torch.from_numpy(q), trainable=True)
    elif kind in ("benes", "sine"):
        # VDP with the per-dimension non-polynomial drifts (the review's "VDP with Benes / sine"; sde.py:227-312), d = 2
        d = 2
        o_sde, g_sde = _theta_sdes(kind, d, np.array([0.7, 0.4]))
    else:
        d = 1
        w = (rng.normal(size=(1, 3)), 0.1 * rng.normal(size=3), rng.normal(size=(3, 1)), np.zeros(1))
        o_sde, g_sde = np_sde.MLPDriftSDE(w), gsde.MLPDrift(weights=[torch.from_numpy(np.asarray(x)) for x in w])
    smooth = kind.startswith("vanderpol")
    idx = np.arange(4, T - 1, 6)
    y = rng.normal(size=(1, len(idx), d))
    cholR = 0.5 * np.eye(d)
    init = (np.zeros(d), 0.6 * np.eye(d))
    g = VariationalMarkovGPQuadrature((grid[idx], dev(y)), g_sde, grid, MultivariateGaussian(dev(cholR)), prior_initial_state=init)
    o = np_models.VariationalMarkovGP(idx, y[0], o_sde, grid, np_models.MultivariateGaussianLik(cholR), *init)
    # (Van der Pol: the oracle's gradient is exact -- Gaussian identities on a polynomial drift; the network drift's is a difference quotient)
    tol = dict(rtol=1e-8 if smooth else 2e-5, scale_atol=1e-9 if smooth else 2e-6)
    for it in range(4):
        mS = g._forward_packed()
        m, S = o.forward_pass()
        gm, gS = g._natural(mS)
        assert_close(host(gm)[0], m, rtol=1e-9)
        assert_close(host(gS)[0], S, rtol=1e-9)
        np.testing.assert_allclose(float(g.E_sde(mS)[0]), o.E_sde(m[:-1], S[:-1]), rtol=1e-10)
        dm, dS = g._grad_E_sde(mS)
        odm, odS = o._grad_E_sde(m, S)
        assert_close(host(dm)[0], odm, **tol)
        assert_close(host(dS)[0], odS, **tol)
        g.update_lagrange(mS)
        o.update_lagrange(m, S)
        assert_close(host(g.psi_lagrange)[0], o.psi, **tol)
        assert_close(host(g.lambda_lagrange)[0], o.lam, **tol)
        g.update_param(mS, lr=0.1)
        o.update_param(m, S, 0.1)
        assert_close(host(g.A)[0], o.A, **tol)
        assert_close(host(g.b)[0], o.b, **tol)
        if it > 1:
            g.update_initial_statistics(0.1)
            o.update_initial_statistics(0.1)
        np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-8 if smooth else 1e-4)
    if kind.startswith("vanderpol"):
        # d E_sde / d (a, tau) on the path m[1:], S[1:] (vi_sde.py:457-470) against a fourth-order quotient of the oracle's E_sde
        got = g.grad_prior_sde_params()
        m, S = o.forward_pass()

        def e_at(a, tau):
            return np_sde.squared_drift_difference_along_gaussian_path(np_sde.VanderPolSDE(a, tau, q), -o.A, o.b, m[1:], S[1:], dt)
        h = 1e-3
        fd = lambda f: (8 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12 * h)
        np.testing.assert_allclose(got, [fd(lambda e: e_at(1.3 + e, 0.9)), fd(lambda e: e_at(1.3, 0.9 + e))], rtol=1e-7)


def test_prior_learning_recovers_the_oscillator(amd):
    """f-4, learning with a coupled drift: a Van der Pol oscillator (a, tau) = (1.0, 2.0) is simulated (Euler-Maruyama), observed densely
    with small noise, and the drift parameters are learnt from (1.6, 1.2) by both trainers' optimize_prior_sde on the HIP quadrature
    kernels (cvi_dp_trainer.py:207-250: Adam on d(KL - VE)/d(a, tau); vi_markov_gp_trainer.py:163-201: Adam on dE_sde/d(a, tau)),
    alternating with inference: the ELBO goes up and both parameters end closer to the truth than they started."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.trainers import CVISitesTrainer, VIMarkovGPTrainer
    from vidp_amd.variational_cvi_sde import CVISitesSDEQuadrature
    from vidp_amd.vi_sde import VariationalMarkovGPQuadrature
    rng_ = np.random.default_rng(5)
    T, dt, a0, tau0, qv = 400, 0.01, 1.0, 2.0, 0.05
    x = np.zeros((T, 2))
    x[0] = (1.0, 0.5)
    for t in range(T - 1):
        f = tau0 * np.array([a0 * (x[t, 0] - x[t, 0] ** 3 / 3.0 - x[t, 1]), x[t, 0] / a0])
        x[t + 1] = x[t] + dt * f + np.sqrt(dt * qv) * rng_.normal(size=2)
    grid = np.arange(T) * dt
    idx = np.arange(2, T - 1, 4)
    y = (x[idx] + 0.02 * rng_.normal(size=(len(idx), 2)))[None]
    lik = MultivariateGaussian(dev(0.02 * np.eye(2)))
    init = (x[0].copy(), 0.05 * np.eye(2))
    q = torch.from_numpy(qv * np.eye(2))
    err = lambda s: (abs(s.a - a0), abs(s.tau - tau0))
    # CVI-DP
    sde = gsde.VanderPolOscillatorSDE(1.6, 1.2, q, trainable=True)
    e0 = err(sde)
    m = CVISitesSDEQuadrature(sde, grid, (grid[idx], dev(y)), lik, prior_initial_state=init)
    tr = CVISitesTrainer(m, data_sites_lr=0.9, girsanov_sites_lr=0.5, max_itr=6, max_itr_sites_optim=4, learn_prior_sde=True,
                         prior_sde_lr=0.05, learning_max_itr=25, learning_tol=1e-3, optim_tol=1e-3)
    elbos, _, _, hist = tr.optimize()
    m.plan.check_info()
    e1 = err(sde)
    assert np.isfinite(elbos).all() and elbos[-1] > elbos[1]
    assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1], (e0, e1, hist)
    # VDP
    sde2 = gsde.VanderPolOscillatorSDE(1.6, 1.2, q, trainable=True)
    # (the fixed-point iteration of VDP is stiff under a sharp likelihood -- jumps of -1/2 R^{-1} in psi --: a blunter one for this model)
    v = VariationalMarkovGPQuadrature((grid[idx], dev(y)), sde2, grid, MultivariateGaussian(dev(0.15 * np.eye(2))), prior_initial_state=init,
                                      stabilize_system=True)
    tv = VIMarkovGPTrainer(v, q_lr=0.1, x0_lr=0.05, max_itr=8, warmup_itr=2, learn_prior_sde=True, prior_sde_lr=0.05, learning_max_itr=25,
                           learning_tol=1e-3)
    ev, _, _, hist2 = tv.optimize()
    e2 = err(sde2)
    assert np.isfinite(ev).all()
    assert e2[0] < 0.6 * e0[0] and e2[1] < 0.6 * e0[1], (e0, e2, hist2)


def test_variational_markov_gp_stabilized(amd, rng):
    """stabilize_system (vi_sde.py:186-200, 312-323, 393-397): with a step size and observation precision at which the plain
    fixed-point iteration leaves the clipping ranges, the clipped / NaN-scrubbed iteration follows the oracle's."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGP
    d, B, T, dt = 1, 1, 40, 0.01
    grid = np.arange(T) * dt
    idx = np.arange(3, T - 1, 4)
    y = 3.0 * np.sign(rng.normal(size=(B, len(idx), d)))
    cholR = 0.01 * np.eye(d)                     # R^{-1} = 1e4: the jump conditions exceed CLIP_MAX = 5000
    init = (np.zeros(d), 0.5 * np.eye(d))
    g = VariationalMarkovGP((grid[idx], dev(y)), gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, MultivariateGaussian(dev(cholR)),
                            prior_initial_state=init, stabilize_system=True)
    o = np_models.VariationalMarkovGP(idx, y[0], np_sde.DoubleWellSDE(np.eye(d)), grid, np_models.MultivariateGaussianLik(cholR), *init,
                                      stabilize_system=True)
    plan = g.plan
    clipped = False
    for it in range(4):
        mS = g._forward_packed()
        m, S = o.forward_pass()
        assert_close(host(plan.unpack(amd.VEC, mS[0]))[0], m)
        assert_close(host(plan.unpack(amd.SYM, mS[1]))[0], S)
        g.update_lagrange(mS)
        o.update_lagrange(m, S)
        clipped = clipped or np.abs(o.psi).max() > 5000.0 or np.abs(o.lam).max() > 5000.0
        assert_close(host(plan.unpack(amd.FULL, g.psi_lagrange, T - 1))[0], o.psi)
        assert_close(host(plan.unpack(amd.VEC, g.lambda_lagrange, T - 1))[0], o.lam)
        g.update_param(mS, lr=0.5)                   # clips the multipliers in place before using them
        o.update_param(m, S, 0.5)
        assert_close(host(plan.unpack(amd.FULL, g.psi_lagrange, T - 1))[0], o.psi)
        assert_close(host(plan.unpack(amd.FULL, g.A, T - 1))[0], o.A)
        assert_close(host(plan.unpack(amd.VEC, g.b, T - 1))[0], o.b)
    assert clipped                                   # the scenario does exercise the clipping
    # the clipped transitions T_t, read back from the sub-diagonal precision blocks -W T_t of a forward pass over the precision
    # route (W = 1 / (dt q))
    g.forward_mode = "precision"
    g._forward_packed()
    sub = host(plan.unpack(amd.FULL, g._fw["nat"][2], T - 1))
    ssm_A = np.abs(sub * (g.dt * np.asarray(g.prior_sde.q_diag))[:, None]).max()
    assert ssm_A <= 1.0 + 1e-12


@pytest.mark.parametrize("d,kind,B,T,R0", [(1, "dw", 3, 57, 8), (2, "dw", 2, 61, 8), (3, "ou", 2, 64, 4), (6, "dw", 3, 131, 8), (6, "dw", 1, 33, 16),
                                           (4, "dw", 2, 61, 8), (5, "ou", 2, 64, 4), (7, "dw", 2, 57, 8), (8, "ou", 1, 33, 16)])
def test_fused_girsanov_update_equals_two_kernel_update(amd, rng, d, kind, B, T, R0):
    """
    update_girsanov_sites inside the backward sweep (mfgm_packed_selinv_girsanov) against the refresh + moment-array update
    (mfgm_packed_selinv_mom_s + mfgm_packed_sde_lean mode 3) from the same state: ragged last segments (one node, several
    nodes), several trajectories, two consecutive steps (the second one reads the swapped buffers).
    """
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    dt = 0.02
    q = torch.diag(torch.from_numpy(0.5 + rng.random(d)))
    grid = np.arange(T) * dt
    idx = np.sort(rng.choice(np.arange(1, T), size=7, replace=False))
    y = np.sign(rng.normal(size=(B, 7, d))) + 0.2 * rng.normal(size=(B, 7, d))
    init = (0.3 * rng.normal(size=d), 0.5 * np.eye(d) + 0.1 * np.ones((d, d)))

    cholR = 0.3 * np.eye(d) + 0.1 * np.eye(d, k=-1)          # correlated noise: dense d x d data sites

    def run(fused, cq=True):
        sde = gsde.OrnsteinUhlenbeckSDE(1.2, q) if kind == "ou" else gsde.DoubleWellSDE(q)
        m = CVISitesSDE(sde, grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)), prior_initial_state=init,
                        plan=amd.Plan(B, T, d, R0=R0, Rup=3))
        m.fused_girsanov, m.cq_enabled = fused, cq
        out = []
        for it, (lr_d, lr_g) in enumerate(((0.5, 0.3), (0.3, 0.15), (0.4, 0.2))):
            m.update_data_sites(lr_d)
            m.update_girsanov_sites(lr_g)
            assert (m._cq is not None) == (fused and cq)
            tq = m.full_sites()
            pl = m.plan
            out.append((host(pl.unpack(amd.VEC, tq.lin)), host(pl.unpack(amd.SYM, tq.diag)), host(pl.unpack(amd.FULL, tq.sub, T - 1)),
                        host(m.classic_elbo_per_trajectory()), host(m.fx_mus), host(m.fx_covs), host(m.data_nat1), host(m.data_nat2),
                        host(m.fx_mus_obs), host(m.fx_covs_obs)))
            if it == 1:
                m.relinearize()      # the sites absorb the change of prior: theta_q, hence everything above, is unchanged by it
        return out

    # a: structured (cq) state, the data sites added inside the sweeps; b: two-kernel update on the dense arrays; c: fused sweeps on
    # the dense arrays
    a, b, c = run(True), run(False), run(True, cq=False)
    for sa, sb, sc in zip(a, b, c):
        for xa, xb, xc in zip(sa, sb, sc):
            assert np.isfinite(xa).all()
            np.testing.assert_allclose(xa, xb, rtol=1e-10, atol=1e-11 * max(1.0, np.abs(xb).max()))
            np.testing.assert_allclose(xc, xb, rtol=1e-10, atol=1e-11 * max(1.0, np.abs(xb).max()))


def test_cq_marginals_on_demand(amd, rng, monkeypatch):
    """The cq refresh behind classic_elbo does not write the [B, T] marginal arrays (only the KL sum and the marginals at the observation
    nodes); fx_mus / fx_covs produce them on demand from the factor in place -- also after another factorisation has run on the plan
    (its coarse levels are then stale and the factor is redone) -- and equal the eager route (VIDP_LAZY_MARGINALS=0)."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    d, B, T = 6, 2, 150
    grid = np.arange(T) * 0.02
    idx = np.sort(rng.choice(np.arange(1, T), size=9, replace=False))
    y = np.sign(rng.normal(size=(B, 9, d))) + 0.2 * rng.normal(size=(B, 9, d))
    q = torch.diag(torch.from_numpy(0.5 + rng.random(d)))

    def run(lazy, disturb):
        monkeypatch.setenv("VIDP_LAZY_MARGINALS", "1" if lazy else "0")
        m = CVISitesSDE(gsde.DoubleWellSDE(q), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(0.3 * np.eye(d))),
                        plan=amd.Plan(B, T, d, R0=8, Rup=3))
        for _ in range(2):
            m.update_data_sites(0.5)
            m.update_girsanov_sites(0.3)
        e = host(m.classic_elbo_per_trajectory())
        assert m._cq is not None and (m._q["mu"] is None) == lazy
        if disturb:
            m.dist_q.marginal_means          # another factorisation on the same plan
        return e, host(m.fx_mus), host(m.fx_covs), host(m.fx_mus_obs)

    ref = run(False, False)
    for lazy, disturb in ((True, False), (True, True)):
        got = run(lazy, disturb)
        for a, b in zip(got, ref):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("d,B,T,stab,kind", [(1, 2, 60, False, "dw"), (2, 2, 700, False, "ou"), (3, 1, 140, True, "dw"), (6, 2, 90, True, "dw"),
                                             (5, 3, 400, False, "ou"), (7, 1, 50, False, "ou")])
def test_vdp_lagrange_sweep_with_parameter_update(amd, rng, d, B, T, stab, kind):
    """update_lagrange_and_param (one set of sweeps) against update_lagrange followed by update_param, three consecutive iterations."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGP
    dt = 0.01
    grid = np.arange(T) * dt
    idx = np.arange(5, T - 1, 9)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    # a small observation noise makes the multipliers large enough for stabilize_system to clip them
    lik_chol = (0.02 if stab else 0.5) * np.eye(d)

    def run(fused, lean=False, level=2):
        q = torch.eye(d, dtype=torch.float64)
        VariationalMarkovGP.dense_jumps = not fused      # the two-call form also reads the dense jump-condition array
        # what the moment recursion makes for the Lagrange call on the side: 0 nothing, 1 the A-only products, 2 the offsets too
        VariationalMarkovGP.fuse_lagrange = level
        g = VariationalMarkovGP((grid[idx], dev(y)), gsde.DoubleWellSDE(q) if kind == "dw" else gsde.OrnsteinUhlenbeckSDE(0.9, q), grid,
                                MultivariateGaussian(dev(lik_chol)), prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)),
                                stabilize_system=stab, plan=amd.Plan(B, T, d, R0=8, Rup=3))
        out = []
        for _ in range(3):
            mS = g._forward_packed()
            if fused:
                g.update_lagrange_and_param(mS, lr=0.05, store_multipliers=not lean)
            else:
                g.update_lagrange(mS)
                g.update_param(mS, lr=0.05)
            pl = g.plan
            if lean:
                # the sweep kept the multipliers of node 0 only: (A, b), psi(0), lambda(0) and what update_initial_statistics makes of them
                psi0, lam0 = g._mult0
                if not stab:        # (clipped multipliers of +-5000 do not give a positive definite q(x0): the scenario is about clipping)
                    g.update_initial_statistics(0.1)
                out.append([host(pl.unpack(amd.FULL, g.A, T - 1)), host(pl.unpack(amd.VEC, g.b, T - 1)), host(psi0), host(lam0),
                            host(g.q0_mu), host(g.q0_chol)])
            else:
                rec = [host(pl.unpack(amd.FULL, g.A, T - 1)), host(pl.unpack(amd.VEC, g.b, T - 1)),
                       host(pl.unpack(amd.FULL, g.psi_lagrange, T - 1)), host(pl.unpack(amd.VEC, g.lambda_lagrange, T - 1))]
                if not stab:
                    g.update_initial_statistics(0.1)
                out.append(rec + [host(g.q0_mu), host(g.q0_chol)])
        return out

    try:
        ra, rb, rc = run(True), run(False), run(True, lean=True)
        rc1, rc0 = run(True, lean=True, level=1), run(True, lean=True, level=0)
    finally:
        VariationalMarkovGP.dense_jumps = False
        VariationalMarkovGP.fuse_lagrange = 2
    for sc, s1, s0 in zip(rc, rc1, rc0):
        for xc, x1, x0 in zip(sc, s1, s0):
            np.testing.assert_allclose(x1, x0, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(x0).max()))
            np.testing.assert_allclose(xc, x0, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(x0).max()))
    for sa, sb, sc in zip(ra, rb, rc):
        for xa, xb in zip(sa, sb):
            assert np.isfinite(xb).all()
            np.testing.assert_allclose(xa, xb, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(xb).max()))
        # lean form: A, b | psi(0), lambda(0) | q(x0)
        for xc, xb in zip(sc, [sb[0], sb[1], sb[2][:, 0], sb[3][:, 0], sb[4], sb[5]]):
            np.testing.assert_allclose(xc, xb, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(xb).max()))


def test_full_size_fused_model_steps(amd):
    """
    Headline size (B = 64, T = 100k, d = 6; the bench workload): two CVI-DP steps with the Girsanov update and the KL sum made inside
    the backward sweeps against the same steps through the moment array, and one VDP step with the parameter update made inside the
    Lagrange sweep against the two separate calls.  Per-trajectory ELBOs must agree: a property that does not need the CPU oracle.
    """
    import gc
    import torch
    import bench
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    from vidp_amd.vi_sde import VariationalMarkovGP
    B, T, d, dt, noise = 64, 100000, 6, 0.01, 0.1
    idx, ys = bench.synth_double_well(B, T, d, dt, 50, noise, seed=5)
    grid = np.arange(T) * dt
    dev_ = torch.device("cuda", 0)
    lik = lambda: MultivariateGaussian(torch.from_numpy(bench.obs_chol(d, noise)).to(dev_))
    q = torch.eye(d, dtype=torch.float64)

    def cvi(fused):
        m = CVISitesSDE(gsde.DoubleWellSDE(q=q), grid, (grid[idx], torch.from_numpy(ys).to(dev_)), lik(),
                        prior_initial_state=(np.zeros(d), np.eye(d)), plan=amd.Plan(B, T, d))
        m.fused_girsanov = fused
        out = []
        for _ in range(2):
            m.update_data_sites(0.5)
            m.update_girsanov_sites(0.1)
            out.append(host(m.classic_elbo_per_trajectory()))
        m.plan.check_info()
        return out

    a = cvi(True)
    gc.collect(); torch.cuda.empty_cache()
    b = cvi(False)
    gc.collect(); torch.cuda.empty_cache()
    for ea, eb in zip(a, b):
        assert np.isfinite(ea).all()
        np.testing.assert_allclose(ea, eb, rtol=1e-9)

    def vdp(fused):
        m = VariationalMarkovGP((grid[idx], torch.from_numpy(ys).to(dev_)), gsde.DoubleWellSDE(q=q), grid, lik(),
                                prior_initial_state=(np.zeros(d), np.eye(d)), stabilize_system=True, plan=amd.Plan(B, T, d))
        m.plan.pack(amd.FULL, (4.0 * torch.eye(d, dtype=torch.float64, device=dev_)).expand(B, T, d, d).contiguous(), out=m.A)
        mS = m._forward_packed()
        if fused:
            m.update_lagrange_and_param(mS, lr=0.01)
        else:
            m.update_lagrange(mS)
            m.update_param(mS, lr=0.01)
        e = host(m.elbo_per_trajectory(m._forward_packed()))
        m.plan.check_info()
        return e

    ea = vdp(True)
    gc.collect(); torch.cuda.empty_cache()
    eb = vdp(False)
    assert np.isfinite(ea).all()
    np.testing.assert_allclose(ea, eb, rtol=1e-9)


def test_site_lerp_kernel(amd, rng):
    """mfgm_site_lerp (variational_cvi.py:364-368: both site variables assigned (1 - rho) theta + rho g) against the torch formula, on
    arrays of different lengths; and CVIGaussianProcess.update_sites, which calls it behind torch's back, must still move the version
    counters the factor caches are keyed on."""
    import torch
    from vidp_amd import _lib
    from vidp_amd.packed import _ptr, _stream
    for n1, n2 in ((1, 1), (1000, 1000), (70001, 13), (5, 300000)):
        x1, g1, x2, g2 = (dev(rng.normal(size=n)) for n in (n1, n1, n2, n2))
        r1, r2 = torch.lerp(x1, g1, 0.3), torch.lerp(x2, g2, 0.3)
        _lib.check(_lib.load().mfgm_site_lerp(_ptr(x1), _ptr(g1), n1, _ptr(x2), _ptr(g2), n2, 0.3, _stream()), "mfgm_site_lerp")
        np.testing.assert_allclose(host(x1), host(r1), rtol=1e-15, atol=1e-16)
        np.testing.assert_allclose(host(x2), host(r2), rtol=1e-15, atol=1e-16)
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t = np.linspace(0, 10, 200) + rng.uniform(0, 0.02, size=200)
    y = np.sin(t)[:, None] + 0.1 * rng.normal(size=(200, 1))
    m = CVIGaussianProcess((dev(t), dev(y)), K.Matern52(1.0, 1.0), Gaussian(0.1), learning_rate=0.5)
    v = (m.sites.nat1._version, m.sites.nat2._version)
    e0 = float(m.classic_elbo())
    m.update_sites()
    assert m.sites.nat1._version > v[0] and m.sites.nat2._version > v[1]
    assert abs(float(m.classic_elbo()) - e0) > 1e-6 * abs(e0)


def test_full_size_steps_against_the_c_port(amd):
    """
    Headline size (B = 64, T = 100k, d = 6) and config 3 (VDP, T = 50k) against the ORACLE: the plain-C port of the same steps
    (oracle/csrc/btd_ref.c: ref_cvi_dp_step / ref_vdp_step, sequential block sweeps, no partition) run on the first 8 trajectories of
    the same data.  Per-trajectory ELBOs after each of two steps must agree to 1e-9 (north-star bound 1e-5): the partitioned HIP
    sweeps, the structured state and the fused site updates at the size the bench measures, checked against an independent CPU
    restatement rather than against themselves.
    """
    import gc
    import torch
    import bench
    from oracle import c_ref
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    from vidp_amd.vi_sde import VariationalMarkovGP
    B, d, dt, noise, Bs = 64, 6, 0.01, 0.1, 8
    dev_ = torch.device("cuda", 0)
    Lc = bench.obs_chol(d, noise)
    Rinv, logdetR = np.linalg.inv(Lc @ Lc.T), 2 * np.sum(np.log(np.diag(Lc)))
    lik = lambda: MultivariateGaussian(torch.from_numpy(Lc).to(dev_))
    q = torch.eye(d, dtype=torch.float64)

    # CVI-DP, headline size
    T = 100000
    idx, ys = bench.synth_double_well(B, T, d, dt, 50, noise, seed=11)
    grid = np.arange(T) * dt
    m = CVISitesSDE(gsde.DoubleWellSDE(q=q), grid, (grid[idx], torch.from_numpy(ys).to(dev_)), lik(),
                    prior_initial_state=(np.zeros(d), np.eye(d)), plan=None)
    assert m.plan.R == 100          # the model's own partition: segments aligned with the observation grid (every 50 nodes)
    got = []
    for _ in range(2):
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.1)
        got.append(host(m.classic_elbo_per_trajectory())[:Bs])
    m.plan.check_info()
    del m
    gc.collect(); torch.cuda.empty_cache()
    alpha, beta = 1.0 + dt * 4.0, dt * 4.0
    A = np.broadcast_to((alpha - 3.0 * beta) * np.eye(d), (T - 1, d, d))           # the prior linearised on N(0, I), as the model starts
    chol = np.concatenate([np.eye(d)[None], np.broadcast_to(np.sqrt(dt) * np.eye(d), (T - 1, d, d))], axis=0)
    lin, diag, sub = c_ref.ssm_to_naturals(A, np.zeros((T, d)), chol)
    rep = lambda a: np.broadcast_to(a, (Bs,) + a.shape).copy()
    st = c_ref.CviDpStepState(rep(lin), rep(diag), rep(sub), idx, ys[:Bs], Rinv, logdetR, alpha, beta, np.ones(d), dt, np.zeros(d), np.eye(d))
    for k in range(2):
        st.step(0.5, 0.1)
        assert np.isfinite(st.elbo).all()
        np.testing.assert_allclose(got[k], st.elbo, rtol=1e-9)
    del st

    # VDP, config 3 size
    T = 50000
    idx, ys = bench.synth_double_well(B, T, d, dt, 50, noise, seed=12)
    grid = np.arange(T) * dt
    m = VariationalMarkovGP((grid[idx], torch.from_numpy(ys).to(dev_)), gsde.DoubleWellSDE(q=q), grid, lik(),
                            prior_initial_state=(np.zeros(d), np.eye(d)), stabilize_system=True, plan=None)
    m.plan.pack(amd.FULL, (4.0 * torch.eye(d, dtype=torch.float64, device=dev_)).expand(B, T, d, d).contiguous(), out=m.A)
    mS = m._forward_packed()
    got = []
    for _ in range(2):
        m.update_lagrange_and_param(mS, lr=0.01)
        mS = m._forward_packed()
        got.append(host(m.elbo_per_trajectory(mS))[:Bs])
    m.plan.check_info()
    sv = c_ref.VdpStepState(np.broadcast_to(4.0 * np.eye(d), (Bs, T - 1, d, d)), np.zeros((Bs, T - 1, d)), idx, ys[:Bs], Rinv, logdetR, 4.0, 4.0,
                            np.ones(d), dt, np.zeros(d), np.eye(d), stabilize=True)
    for k in range(2):
        sv.step(0.01)
        assert np.isfinite(sv.elbo).all()
        np.testing.assert_allclose(got[k], sv.elbo, rtol=1e-9)


@pytest.mark.parametrize("streams", [False, True])
def test_cvi_dp_pipelined_steps_equal_unpipelined(amd, rng, streams):
    """The cross-step pipelining of CVISitesSDE (the level-0 reduce of the next step's first factorisation made ahead by
    mfgm_cq_factor_pipelined: as the second wavefront of the forward sweep's workgroups, k_forward_reduce_cq, or on a second stream,
    k_reduce_cq_lean) against the same model with it switched off: ELBO after every step of a loop that keeps its
    learning rates (records are consumed), changes them (a record is dropped), re-linearises, evaluates the ELBO twice and updates
    the Girsanov sites twice in a row -- equal to rounding of the last bit (the record holds the numbers the reduce would write).
    Then three ways of invalidating a record that a classic_elbo has just made, each followed by two ordinary steps: "x" another
    factorisation on the model's plan, "a" a new tensor assigned to data_nat1, "i" data_nat1 edited in place through torch.  The next
    update_data_sites must not take the record over."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    B, T, d, dt = 3, 1200, 3, 0.01
    grid = np.arange(T) * dt
    idx = np.arange(9, T - 1, 20)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    cholR = 0.3 * np.eye(d)

    def make(pipe):
        m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)),
                        prior_initial_state=(np.zeros(d), np.eye(d)), plan=amd.Plan(B, T, d, R0=20, Rup=4))
        m.pipelined = pipe
        m.pipeline_min_nodes = 0          # (the model pipelines from 200 000 nodes on: this chain is short)
        return m
    a, b = make(False), make(True)
    b.pipe_two_streams = streams          # the reduce made ahead: second wavefront of the forward kernel / kernel of its own on a second stream
    assert b._cq_state() is not None
    prog = [("s", 0.5, 0.1)] * 4 + [("s", 0.3, 0.1)] * 2 + [("r",)] + [("s", 0.3, 0.2)] * 2 + [("e",), ("g", 0.1), ("s", 0.3, 0.2), ("s", 0.3, 0.2)]
    more = [("x",), ("s", 0.3, 0.2), ("s", 0.3, 0.2), ("a",), ("s", 0.3, 0.2), ("s", 0.3, 0.2), ("i",), ("s", 0.3, 0.2), ("s", 0.3, 0.2)]
    got, want, used, held = [], [], None, None
    for k, op in enumerate(prog + more):
        if k == len(prog):
            used = b._ahead.consumed
        for m, out in ((a, want), (b, got)):
            if op[0] == "s":
                m.update_data_sites(op[1])
                if m is b and held is not None:
                    assert b._ahead.consumed == held      # the record made before the "x" / "a" / "i" was not taken over
                    held = None
                m.update_girsanov_sites(op[2])
            elif op[0] == "r":
                m.relinearize()
            elif op[0] == "g":
                m.update_girsanov_sites(op[1])
            elif op[0] == "x":
                tp = m._theta_p
                m.plan.factor(tp.diag, tp.sub, tp.lin, aD=-2.0, aS=-1.0)
            elif op[0] == "a":
                m.data_nat1 = m.data_nat1 * 0.9
                assert m._cq.site_lin is m.data_nat1
            elif op[0] == "i":
                m.data_nat1.mul_(1.1)
                m._sites_moved()
            if op[0] in "xai":
                if m is b:
                    assert b._ahead.rec is not None       # (the ELBO of the step before made one)
                    held = b._ahead.consumed
                continue                                  # (an ELBO here would make a record for the new state)
            out.append(host(m.classic_elbo_per_trajectory()))
    b.plan.check_info()
    assert used >= 6                    # records were made and consumed, not just dropped
    assert b._ahead.consumed > used     # ... also after the invalidations
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=1e-12)
    assert_close(host(b.plan.unpack(amd.VEC, b.full_sites().lin)), host(a.plan.unpack(amd.VEC, a.full_sites().lin)), rtol=1e-12)


def test_full_size_cvigp_and_sparse_steps_against_the_c_port(amd):
    """
    Config 2 at FULL size (CVIGaussianProcess.update_sites + elbo, Matern-5/2, one chain of 100 000 points; reference
    variational_cvi.py:351-379) against the C port's ref_cvigp_step, and config 5's model step (SparseCVIGaussianProcess.update_sites +
    classic_elbo, Sum-of-Matern d = 16; reference sparse_variational_cvi.py:140-221) against ref_sparse_cvi_step on the SAME 40 000
    inducing states / 80 000 observations (the largest problem the one-thread port finishes in under a minute; nothing is scaled):
    ELBO after each of three damped steps, 1e-8 (north-star bound 1e-5).
    """
    import gc
    import torch
    import bench
    from oracle import c_ref, np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    dev_ = torch.device("cuda", 0)

    # config 2, full size: bench.bench_cvigp's recipe
    T = 100000
    rng_ = np.random.default_rng(71892305 + 2)
    t = torch.linspace(0, 0.01 * T, T, dtype=torch.float64, device=dev_)
    y = (torch.sin(12 * t) + 0.1 * torch.from_numpy(rng_.normal(size=T)).to(dev_))[:, None]
    m = CVIGaussianProcess((t, y), K.Matern52(lengthscale=0.2, variance=1.0), Gaussian(0.01), learning_rate=0.5)
    got = []
    for _ in range(3):
        m.update_sites()
        got.append(float(m.elbo()))
    m.dist_p.plan.check_info()
    k = np_kernels.Matern52(0.2, 1.0)
    tn = t.cpu().numpy()
    st = c_ref.CviGpStepState(k.state_space_model(tn), k.emission_matrix(tn[:1])[0, 0], y.cpu().numpy(), 0.01, 0.5)
    want = [st.step() for _ in range(3)]
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-8)
    del m, st
    gc.collect(); torch.cuda.empty_cache()

    # config 5 on the same bounded problem on both sides
    sample = 40000
    got = bench.c5_gpu_elbos(sample, 3, dev_)
    z, ts, ys = bench.c5_sample_problem(sample)
    st = c_ref.SparseCviStepState(bench.sum16_kernel(np_kernels), z, ts, ys, 0.01, 0.5)
    want = [st.step() for _ in range(3)]
    assert np.isfinite(want).all() and want[2] > want[0]
    np.testing.assert_allclose(got, want, rtol=1e-8)


@pytest.mark.parametrize("d,B,T,n_obs", [(1, 2, 40, 5), (3, 3, 77, 9), (6, 2, 131, 300)])
def test_site_update_and_obs_ve_kernels(amd, rng, d, B, T, n_obs):
    """mfgm_site_update_pair and mfgm_mvn_obs_ve against the torch formulas they replace (blend + difference + scatter; gather +
    multivariate-Gaussian variational expectations + per-trajectory sum)."""
    import math
    import torch
    from vidp_amd.likelihoods import MultivariateGaussian
    n_obs = min(n_obs, T - 1)
    plan = amd.Plan(B, T, d, R0=8, Rup=3)
    ti = np.stack([np.sort(rng.choice(T, size=n_obs, replace=False)) for _ in range(B)])
    ids = plan.node_ids(ti)
    n = B * n_obs
    lin0, diag0 = dev(rng.normal(size=(B, T, d))), dev(rng.normal(size=(B, T, d, d)))
    diag0 = diag0 + diag0.transpose(-1, -2)
    pv, ps = plan.pack(amd.VEC, lin0), plan.pack(amd.SYM, diag0)
    s1, s2 = dev(rng.normal(size=(n, d))), dev(rng.normal(size=(n, d, d)))
    s2 = (s2 + s2.transpose(-1, -2)).contiguous()
    g1, g2 = dev(rng.normal(size=(n, d))), dev(rng.normal(size=(n, d, d)))
    g2 = (g2 + g2.transpose(-1, -2)).contiguous()
    lr = 0.3
    new1, new2 = (1 - lr) * s1 + lr * g1, (1 - lr) * s2 + lr * g2
    ref_v, ref_s = pv.clone(), ps.clone()
    plan.scatter_nodes_pair(ref_v, ref_s, ids, new1 - s1, new2 - s2)
    a1, a2 = s1.clone(), s2.clone()
    plan.site_update_pair(pv, ps, ids, a1, a2, g1, g2, lr)
    np.testing.assert_allclose(host(a1), host(new1), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(host(a2), host(new2), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(host(plan.unpack(amd.VEC, pv)), host(plan.unpack(amd.VEC, ref_v)), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(host(plan.unpack(amd.SYM, ps)), host(plan.unpack(amd.SYM, ref_s)), rtol=1e-13, atol=1e-14)

    # variational expectations at the observation nodes
    cov = dev(rng.normal(size=(B, T, d, d)))
    cov = cov @ cov.transpose(-1, -2) + 0.5 * torch.eye(d, dtype=torch.float64, device="cuda")
    mu = dev(rng.normal(size=(B, T, d)))
    pm, pc = plan.pack(amd.VEC, mu), plan.pack(amd.SYM, cov)
    cholR = np.linalg.cholesky(0.2 * np.eye(d) + 0.05 * np.ones((d, d)))
    lik = MultivariateGaussian(dev(cholR))
    y = dev(rng.normal(size=(n, d)))
    om, oc = torch.empty((n, d), dtype=torch.float64, device="cuda"), torch.empty((n, d, d), dtype=torch.float64, device="cuda")
    cst = -float(lik.log_det_chol) - 0.5 * d * math.log(2.0 * math.pi)
    ve = plan.mvn_obs_ve(pm, pc, ids, n_obs, y, lik.inv_covariance, cst, out_mu=om, out_cov=oc)
    gm, gc = plan.gather_nodes(amd.VEC, pm, ids), plan.gather_nodes(amd.SYM, pc, ids)
    np.testing.assert_array_equal(host(om), host(gm))
    np.testing.assert_array_equal(host(oc), host(gc))
    ref = lik.variational_expectations(gm, gc, y).reshape(B, n_obs).sum(-1)
    np.testing.assert_allclose(host(ve), host(ref), rtol=1e-12)


@pytest.mark.parametrize("d,B,T,stab", [(1, 2, 60, False), (2, 3, 700, False), (3, 2, 141, True), (6, 2, 90, False)])
def test_vdp_forward_pass_routes_agree(amd, rng, d, B, T, stab):
    """forward_pass as the partitioned moment recursion, over precision blocks + factorisation + selected inverse, and over explicit
    SSM arrays: the same marginals (per-trajectory q(x0), random contractive drifts, ragged last segment, > 64 segments)."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGP
    dt = 0.01
    grid = np.arange(T) * dt
    idx = np.arange(5, T - 1, 9)
    y = rng.normal(size=(B, len(idx), d))
    g = VariationalMarkovGP((grid[idx], dev(y)), gsde.OrnsteinUhlenbeckSDE(0.9, torch.eye(d, dtype=torch.float64)), grid,
                            MultivariateGaussian(dev(0.5 * np.eye(d))), prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)),
                            stabilize_system=stab, plan=amd.Plan(B, T, d, R0=8, Rup=3))
    A = 3.0 * rng.normal(size=(B, T, d, d)) + 4.0 * np.eye(d)
    b = (120.0 if stab else 2.0) * rng.normal(size=(B, T, d))          # stabilised: offsets dt b beyond [-1, 1] are clipped
    if stab:
        # some strictly upper-triangular entries of I - dt A leave [-1, 1] and are clipped, a few are NaN and become 1e-8; the
        # transitions stay (non-normal but) contractive, as a chain the clipping is meant to rescue
        A = np.triu(A)
        mask = np.triu(rng.random((B, T, d, d)) < 0.15, 1)
        A = np.where(mask, 150.0 * np.sign(rng.normal(size=A.shape)), A)
        A = np.where(np.triu(rng.random((B, T, d, d)) < 0.02, 1), np.nan, A)
    g.plan.pack(amd.FULL, dev(A), out=g.A)
    g.plan.pack(amd.VEC, dev(b), out=g.b)
    g.q0_mu = dev(rng.normal(size=(B, d)))
    L0 = np.tril(rng.normal(size=(B, d, d)), -1) * 0.2 + np.eye(d) * (0.5 + rng.random((B, d, 1)))
    g.q0_chol = dev(L0)
    out = {}
    for mode in ("moments", "precision", "ssm"):
        g.forward_mode = mode
        m, S = g.forward_pass
        g.plan.check_info()
        out[mode] = (host(m), host(S))
    for mode in ("precision", "ssm"):
        for xa, xb in zip(out["moments"], out[mode]):
            assert np.isfinite(xa).all()
            np.testing.assert_allclose(xa, xb, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(xb).max()))


def test_vdp_esde_from_the_forward_sweep(amd, rng):
    """E_sde returned by the forward pass's final sweep equals the stand-alone kernel on the same marginals, and the cached value is
    dropped when (A, b) or the drift parameters change."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGP
    d, B, T, dt = 3, 3, 150, 0.01
    grid = np.arange(T) * dt
    idx = np.arange(5, T - 1, 9)
    y = rng.normal(size=(B, len(idx), d))
    g = VariationalMarkovGP((grid[idx], dev(y)), gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid,
                            MultivariateGaussian(dev(0.5 * np.eye(d))), prior_initial_state=(np.zeros(d), 0.5 * np.eye(d)),
                            plan=amd.Plan(B, T, d, R0=8, Rup=3))
    g.plan.pack(amd.FULL, dev(3.0 * rng.normal(size=(B, T, d, d)) + 4.0 * np.eye(d)), out=g.A)
    g.plan.pack(amd.VEC, dev(rng.normal(size=(B, T, d))), out=g.b)
    mS = g._forward_packed()
    fused = host(g.E_sde(mS))
    g._esde_of = None
    np.testing.assert_allclose(fused, host(g.E_sde(mS)), rtol=1e-12)
    # a parameter update invalidates the by-product: E_sde of the OLD marginals under the NEW (A, b) is recomputed
    mS = g._forward_packed()
    g.update_lagrange_and_param(mS, lr=0.05)
    after = host(g.E_sde(mS))
    g._esde_of = None
    np.testing.assert_allclose(after, host(g.E_sde(mS)), rtol=1e-12)
    assert np.abs(after - fused).max() > 1e-6 * np.abs(fused).max()


def test_config1_shipped_data_and_recipe(amd):
    """BASELINE config 1 as SURVEY 8d specifies it, on the reference's own shipped data (docs/diffusion_processes/data.zip member
    data/linear/15/0.npz, committed as tests/golden/linear_15_0.npz) read through exp_io.load_exp_data (exp_dp_utils.py:108-125):
    T = 1001, dt = 0.01, 32 observations, sigma = 0.1, OU prior with decay 1.2 against data generated with decay 0.5, both learning
    rates 1, one site iteration (configs/cvi_linear_process.yaml; README.md:43).  KA11: the ELBO is the closed-form log marginal
    likelihood; the oracle model agrees; NLPD / RMSE on the 8 held-out points follow exp_dp_utils.py:189-224."""
    import os
    import torch
    from oracle import np_sde
    from tests.conftest import GOLDEN
    from tests.test_oracle_models import config1_closed_form_log_marginal, load_config1
    from vidp_amd import exp_io
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.trainers import CVISitesTrainer
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    Q, x0, noise_stddev, latent, observations, time_grid, test_obs = exp_io.load_exp_data(os.path.join(GOLDEN, "linear_15_0.npz"))
    c = load_config1()
    assert time_grid.shape == (1001,) and observations[1].shape == (32, 1) and test_obs[1].shape == (8, 1) and noise_stddev.shape == (1, 1)
    decay, Qv, sigma = 1.2, float(Q), float(noise_stddev.item())
    sde = gsde.OrnsteinUhlenbeckSDE(decay, Qv * torch.eye(1, dtype=torch.float64))
    init = (np.zeros(1), Qv / (2 * decay) * np.eye(1))                              # cvi_dp.py:60-65
    lik = MultivariateGaussian(dev(sigma * np.eye(1)))                              # cvi_dp.py:76
    m = CVISitesSDE(sde, time_grid.cpu().numpy(), observations, lik, prior_initial_state=init)
    tr = CVISitesTrainer(m, test_data=test_obs, girsanov_sites_lr=1.0, data_sites_lr=1.0, max_itr=1, max_itr_sites_optim=1)
    elbos, nlpds, rmses, _ = tr.optimize()
    target = config1_closed_form_log_marginal(c["time_grid"], c["obs_index"], c["y"], decay, Qv, sigma)
    np.testing.assert_allclose(elbos[-1], target, rtol=1e-6)
    o = np_models.CVISitesSDE(np_sde.OrnsteinUhlenbeckSDE(decay, Qv * np.eye(1)), c["time_grid"], c["obs_index"], c["y"],
                              np_models.MultivariateGaussianLik(sigma * np.eye(1)), *init)
    o.update_data_sites(1.0)
    o.update_girsanov_sites(1.0)
    np.testing.assert_allclose(elbos[-1], o.classic_elbo(), rtol=1e-6)
    assert_close(host(m.fx_mus)[0], o.fx_mus)
    assert_close(host(m.fx_covs)[0], o.fx_covs)
    # held-out metrics (exp_dp_utils.py:189-224): y* ~ N(m, S + sigma^2) at the test grid points
    ti = np.searchsorted(c["time_grid"], c["test_grid"])
    mt, St = o.fx_mus[ti, 0], o.fx_covs[ti, 0, 0] + sigma ** 2
    nlpd = -np.mean(-0.5 * np.log(2 * np.pi * St) - 0.5 * (c["test_y"][:, 0] - mt) ** 2 / St)
    rmse = np.sqrt(np.mean((c["test_y"][:, 0] - mt) ** 2))
    np.testing.assert_allclose(nlpds[-1], nlpd, rtol=1e-6)
    np.testing.assert_allclose(rmses[-1], rmse, rtol=1e-6)


def test_likelihood_gradient_cache_is_not_keyed_on_addresses(amd, rng):
    """One likelihood object shared by models whose observation tensors are freed and re-allocated (the caching allocator returns
    the same address for the same shape): the cached S^{-1} y must follow the tensor, not its address."""
    import torch
    from vidp_amd.likelihoods import MultivariateGaussian
    d, n = 3, 50
    lik = MultivariateGaussian(dev(0.4 * np.eye(d)))
    cov = torch.eye(d, dtype=torch.float64, device="cuda").expand(n, d, d).contiguous()
    mu = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    seen = []
    for trial in range(4):
        y = dev(rng.normal(size=(n, d)))
        seen.append(y.data_ptr())
        g1, _ = lik.ve_gradients_expectation(mu, cov, y)
        np.testing.assert_allclose(host(g1), host(y) / 0.16, rtol=1e-12)
        y.mul_(2.0)                                       # in-place edit: same object, new version
        g1, _ = lik.ve_gradients_expectation(mu, cov, y)
        np.testing.assert_allclose(host(g1), host(y) / 0.16, rtol=1e-12)
        del y, g1
    assert len(set(seen)) < len(seen), "the allocator did not reuse an address: the test exercised nothing"
    lik.chol_covariance = dev(0.5 * np.eye(d))            # replacing the factor rebuilds the inverse and drops the cache
    y = dev(rng.normal(size=(n, d)))
    np.testing.assert_allclose(host(lik.ve_gradients_expectation(mu, cov, y)[0]), host(y) / 0.25, rtol=1e-12)


def test_bench_gpus_2_launches_two_ranks(amd):
    """`python bench.py --gpus 2` (no torch.distributed environment) starts two ranks itself -- here over gloo on the one GPU of the
    box, VIDP_DIST_BACKEND=gloo -- reports n_gpus == 2, and its all-reduced ELBO is the sum of two single-rank runs on the same two
    shards of trajectories."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["VIDP_DIST_BACKEND"] = "gloo"
    common = ["--steps", "2", "--warmup", "1", "--B", "4", "--T", "2000", "--no-cpu-baseline", "--no-vdp"]

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra + common, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])

    two = run(["--gpus", "2"])
    assert two["n_gpus"] == 2 and two["config"]["total_trajectories"] == 8 and two["scaling"] == "weak"
    singles = [run(["--gpus", "1", "--data-rank", str(r)]) for r in range(2)]
    assert all(s["n_gpus"] == 1 for s in singles)
    np.testing.assert_allclose(two["elbo_last"], sum(s["elbo_last"] for s in singles), rtol=1e-12)


def test_bench_dump_outputs_repeat(amd, tmp_path):
    """`python bench.py --dump-outputs DIR` (small headline workload): the last step's ELBO, observation marginals and data sites as
    float64 .npy files whose ELBO is the line's elbo_last, and two runs with the same arguments write identical arrays."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = {"elbo", "fx_mus_obs", "fx_covs_obs", "data_nat1", "data_nat2"}
    got = []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--B", "4",
                            "--T", "2000", "--dump-outputs", out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 2 and "roofline" not in line and "other_configs" not in line
        arrays = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
        assert set(arrays) == names and all(a.dtype == np.float64 for a in arrays.values())
        assert arrays["fx_mus_obs"].shape == (4 * 39, 6) and arrays["data_nat2"].shape == (4 * 39, 6, 6)
        assert arrays["elbo"].shape == (1,) and arrays["elbo"][0] == line["elbo_last"]
        got.append(arrays)
    for n in names:
        np.testing.assert_array_equal(got[0][n], got[1][n])


@pytest.mark.parametrize("config,extra,shapes", [
    ("c2", [], {"site_nat1": (100000, 1), "site_nat2": (100000, 1, 1)}),
    # c3 unpacks the partitioned arrays: the marginals over all B T nodes, the drift parameters over the B (T - 1) transitions
    ("c3", ["--B", "2"], {"m": (2 * 50000, 6), "S": (29127, 6, 6), "A": (29127, 6, 6), "b": (2 * 49999, 6)}),
    ("c5", ["--c5-M", "2000"], {"site_nat1": (2001, 32), "site_nat2": (1024, 32, 32)})], ids=["c2", "c3", "c5"])
def test_bench_dump_outputs_other_configs(amd, tmp_path, config, extra, shapes):
    """`python bench.py --config c2|c3|c5 --dump-outputs DIR`: the arrays each configuration writes, in float64, finite, the ELBO equal
    to the line's elbo_last; the symmetric blocks (c3's marginal covariances, c5's site precisions) come out symmetric, i.e. unpacked in
    the right layout."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / config)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", config, "--steps", "2", "--warmup", "1",
                        "--dump-outputs", out] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    arrays = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
    assert {n: a.shape for n, a in arrays.items()} == dict(shapes, elbo=(1,))
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["elbo"][0] == line["elbo_last"]
    for n in ("S", "site_nat2"):
        if n in arrays and arrays[n].shape[-1] > 1:
            np.testing.assert_allclose(arrays[n], np.swapaxes(arrays[n], -1, -2), rtol=0, atol=1e-12 * np.abs(arrays[n]).max())
    if config == "c3":
        assert np.all(np.linalg.eigvalsh(arrays["S"]) > 0)


def test_bench_c5_gpus_2_is_one_shared_chain(amd):
    """`python bench.py --config c5 --gpus 2`: config 5 as BASELINE states it -- ONE chain shared between the ranks (gloo on the one GPU
    here), strong scaling -- and its ELBO equals the single-GPU run's on the same chain."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["VIDP_DIST_BACKEND"] = "gloo"
    common = ["--config", "c5", "--c5-M", "20000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra + common, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])

    two, one = run(["--gpus", "2"]), run(["--gpus", "1"])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["total_trajectories"] == 1
    assert one["n_gpus"] == 1 and one["scaling"] == "weak"
    np.testing.assert_allclose(two["elbo_last"], one["elbo_last"], rtol=1e-9)


@pytest.mark.parametrize("tag,bs", [("b0", ()), ("b3", (3,))])
def test_kalman_filter_sites_fused_output_dim_2(amd, tag, bs):
    """KA2's fixture (T = 8, d = 3, o = 2, non-zero prior mean) as a filter with per-step sites nat1 = R^{-1} y, nat2 = -1/2 R^{-1}
    through the fused entry points: the log-likelihood equals the reference NumPy filter's, and predict-at-the-data equals
    (H mu, diag H Sigma H^T) of its smoother."""
    from tests.conftest import golden
    from vidp_amd.emission_model import EmissionModel
    from vidp_amd.kalman_filter import GaussianSitesNat, KalmanFilterWithSites
    g = golden(f"kalman_filter_{tag}.npz")
    T = g["y"].shape[-2]
    Rinv = np.linalg.inv(g["R"])
    ssm = _gpu_ssm_from_golden(g, bs, T)
    Hc = dev(g["H"])
    em = EmissionModel(dev(np.broadcast_to(g["H"], bs + (T,) + g["H"].shape).copy()), constant_matrix=Hc)
    y = g["y"].reshape((-1, T, 2))
    B = y.shape[0]
    sites = GaussianSitesNat(dev((y @ Rinv).reshape(B * T, 2)), dev(np.broadcast_to(-0.5 * Rinv, (B * T, 2, 2)).copy()))
    kf = KalmanFilterWithSites(ssm, em, sites)
    np.testing.assert_allclose(float(kf.log_likelihood()), g["log_lik_total"], rtol=1e-7)
    # posterior marginals projected onto f
    from vidp_amd.variational_cvi import GaussianProcessWithSitesBase
    class _M:      # the attributes _predict_f_fused reads
        pass
    m = _M()
    m.dist_p, m.sites, m._emission = ssm, sites, (lambda: em)
    Fmu, Fvar = GaussianProcessWithSitesBase._predict_f_fused(m)
    sm, sc = g["smooth_means"], np.broadcast_to(g["smooth_covs"], bs + g["smooth_covs"].shape)
    assert_close(host(Fmu), np.einsum("ai,...ti->...ta", g["H"], sm))
    assert_close(host(Fvar), np.einsum("ai,...tij,aj->...ta", g["H"], sc, g["H"]))


def test_tape_gradients_through_the_sweeps(amd, rng):
    """vidp_amd.tape: gradients of a non-linear function of the marginals, cross-covariances, log-determinant and KL of a TapeSSM with
    respect to its parameters (through the theta -> eta sweeps, backward = Fisher-vector product) against central differences of
    the same function evaluated without a tape."""
    import torch
    from vidp_amd import tape
    from vidp_amd.state_space_model import StateSpaceModel
    B, T, d = 2, 9, 3
    prm = [dev(a) for a in random_ssm_params(rng, (B,), T, d)]
    prior = StateSpaceModel(*[dev(a) for a in random_ssm_params(rng, (B,), T, d)])
    w = dev(rng.normal(size=(T, d)))

    def fn(q):
        mu, cov = q.marginals
        sub = q.subsequent_covariances()
        return ((mu * w) ** 2).sum() + (cov * cov).sum() + torch.sin(sub).sum() + 0.3 * q.log_det_precision().sum() + q.kl_divergence(prior).sum()

    def value(p):
        mu0, cP0, A, b, cQ = p
        with torch.no_grad():
            return float(fn(tape.TapeSSM(mu0, cP0, A, b, cQ, plan=prior.plan)))

    q = tape.TapeSSM(*[p.clone().requires_grad_(True) for p in prm], plan=prior.plan)
    loss = fn(q)
    grads = torch.autograd.grad(loss, [q.mu0, q.cholP0, q.A, q.b, q.cholQ])
    gen = np.random.default_rng(5)
    for k, (p, g) in enumerate(zip(prm, grads)):
        g = host(g)
        for _ in range(4):
            idx = tuple(gen.integers(0, s) for s in p.shape)
            if k in (1, 4) and idx[-1] > idx[-2]:
                continue              # strictly upper entries of the Cholesky factors are not parameters
            def cd(h):
                up, dn = [x.clone() for x in prm], [x.clone() for x in prm]
                up[k][idx] += h
                dn[k][idx] -= h
                return (value(up) - value(dn)) / (2 * h)
            # fourth-order central difference; the backward pass is exact (congruence scans), so what is left is the rounding of the
            # difference quotient itself (~ eps |f| / h)
            fd = (4.0 * cd(5e-4) - cd(1e-3)) / 3.0
            np.testing.assert_allclose(g[idx], fd, rtol=2e-9, atol=2e-9 * max(1.0, abs(fd)))


def test_ssm_natgrad_tape_route(amd, rng):
    """KA9 through the tape route (ssm_natgrad.py:121-218 with a plain closure): one natural-gradient step with gamma = 1 and a
    Gaussian likelihood makes the variational ELBO equal to the GPR log-likelihood, and the closure's d loss / d eta equals the
    closed-form one of GaussMarkovELBO."""
    import torch
    from oracle import np_kernels
    from vidp_amd import kernels as K, tape
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.ssm_natgrad import GaussMarkovELBO, SSMNaturalGradient
    from vidp_amd.state_space_model import StateSpaceModel
    T, noise = 10, 0.3
    mk = lambda m: m.Sum([m.Matern32(1.1, 0.7), m.Matern12(0.5, 1.2)])
    gk = mk(K)
    d = gk.state_dim
    t = np.sort(rng.uniform(0, 4, size=T))
    y = np.cos(3 * t)[:, None] + 0.1 * rng.normal(size=(T, 1))
    p = gk.state_space_model(dev(t))
    em = gk.generate_emission_model(dev(t))
    lik = Gaussian(noise)
    q = StateSpaceModel(*[dev(a) for a in random_ssm_params(rng, (), T, d)], plan=p.plan)
    H, yy = em.emission_matrix, dev(y)

    def neg_elbo(qt):                                  # a plain closure: no grad_wrt_expectations
        mu, cov = qt.marginals
        fm = torch.einsum("toi,bti->bto", H, mu)
        fv = torch.einsum("toi,btij,toj->bto", H, cov, H)
        return -(lik.variational_expectations(fm, fv, yy).sum() - qt.kl_divergence(p).sum())

    closed = GaussMarkovELBO(p, em, lik, yy)
    _, (g1, g2, g3) = tape.natgrad_wrt_expectations(neg_elbo, q)
    (cl, cd, cs), _ = closed.grad_wrt_expectations(q)
    pl = q.plan
    # the block parts agree to the accuracy of the Richardson difference (1e-10 of the largest entry); the linear part is the small
    # difference of terms of that size (d/d eta_lin = d/d mu - 2 (d/d Sigma) mu ...), hence a looser absolute floor
    assert_close(host(g1), host(pl.unpack(amd.VEC, cl)), rtol=1e-4, scale_atol=1e-5)
    assert_close(host(g2), host(pl.unpack(amd.SYM, cd)), rtol=1e-7, scale_atol=1e-9)
    assert_close(host(g3), host(pl.unpack(amd.FULL, cs, T - 1)), rtol=1e-7, scale_atol=1e-9)
    SSMNaturalGradient(gamma=1.0, momentum=False).minimize(neg_elbo, q)
    ref = np_models.gpr_log_likelihood(t, y, mk(np_kernels), noise)
    np.testing.assert_allclose(float(closed.elbo(q)), ref, rtol=1e-6, atol=1e-5)


def test_trainers_two_processes_share_the_batch():
    """SURVEY 8e first row with the gradient half of the collective: 2 ranks (gloo, one GPU), 4 trajectories spread 2 + 2, both trainers
    with prior learning -- ELBO / NLPD / RMSE and drift-parameter histories equal the single-process run on all 4 (tests/mp_trainer_shard.py)."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "mp_trainer_shard.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.mark.parametrize("B,T,d", [(2, 9, 3), (1, 130, 2), (3, 33, 6), (1, 2, 1), (2, 60, 8), (66, 5, 4), (2, 41, 7)])
def test_exact_band_of_sigma_dP_sigma(amd, rng, B, T, d):
    """The covariance half of the Fisher-vector product behind `tape.NaturalsToExpectations.backward` (ssm_natgrad.py:142-172 takes it
    from a GradientTape through the banded ops): the band of Sigma dP Sigma from the band of Sigma alone (congruence scans), against the
    dense product on a random SPD block-tri-diagonal precision -- including a badly scaled chain (blocks spanning six orders of
    magnitude), where a finite difference of factorisations has no usable step."""
    import torch
    from vidp_amd import tape
    for scale in (None, "bad"):
        diag, sub = random_dominant_btd(rng, (B,), T, d)
        if scale == "bad":
            sc = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=(B, T, d)))
            diag = sc[..., :, None] * diag * sc[..., None, :]
            sub = sc[:, 1:, :, None] * sub * sc[:, :-1, None, :]
        dPd = rng.normal(size=(B, T, d, d))
        dPd = dPd + np.swapaxes(dPd, -1, -2)
        dPs = rng.normal(size=(B, T - 1, d, d))
        if scale == "bad":
            dPd = sc[..., :, None] * dPd * sc[..., None, :]
            dPs = sc[:, 1:, :, None] * dPs * sc[:, :-1, None, :]
        covs, subs, Xd, Xs = [], [], [], []
        for b in range(B):
            P = np_btd.to_dense(diag[b], sub[b], symmetric=True)
            dP = np_btd.to_dense(dPd[b], dPs[b], symmetric=True)
            S = np.linalg.inv(P)
            X = S @ dP @ S
            blk = lambda M, i, j: M[i * d:(i + 1) * d, j * d:(j + 1) * d]
            covs.append(np.stack([blk(S, t, t) for t in range(T)]))
            subs.append(np.stack([blk(S, t + 1, t) for t in range(T - 1)]))
            Xd.append(np.stack([blk(X, t, t) for t in range(T)]))
            Xs.append(np.stack([blk(X, t + 1, t) for t in range(T - 1)]))
        gd, gs = tape.band_of_sigma_dP_sigma(dev(np.stack(covs)), dev(np.stack(subs)), dev(dPd), dev(dPs))
        assert_close(host(gd), np.stack(Xd), rtol=1e-8)
        assert_close(host(gs), np.stack(Xs), rtol=1e-8)
        # the same through the HIP congruence scans (mfgm_congruence_scan) of a plan with short segments: several levels of maps
        plan = amd.Plan(B, T, d, R0=4)
        hd, hs = tape.band_of_sigma_dP_sigma(dev(np.stack(covs)), dev(np.stack(subs)), dev(dPd), dev(dPs), plan=plan)
        assert_close(host(hd), np.stack(Xd), rtol=1e-8)
        assert_close(host(hs), np.stack(Xs), rtol=1e-8)


@pytest.mark.parametrize("B,T,d", [(1, 40, 12), (2, 9, 16), (1, 130, 17), (1, 100, 30), (3, 5, 32), (2, 33, 9), (1, 2, 24)])
def test_exact_band_of_sigma_dP_sigma_wide_blocks(amd, rng, B, T, d):
    """mfgm_wband_sigma_dP_sigma (block sizes up to 32: natural-layout arrays, MFMA Gram products, segment maps for T > 32) against the
    dense product Sigma dP Sigma on a random SPD block-tri-diagonal precision, and against the torch evaluation of the same recurrences
    (VIDP_TAPE_TORCH_SCAN=1) -- the natural-gradient tape's backward at the reference's d = 30 (tests/integration/test_ssm_natgrad.py)."""
    from vidp_amd import tape
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    dPd = rng.normal(size=(B, T, d, d))
    dPd = dPd + np.swapaxes(dPd, -1, -2)
    dPs = rng.normal(size=(B, T - 1, d, d))
    covs, subs, Xd, Xs = [], [], [], []
    blk = lambda M, i, j: M[i * d:(i + 1) * d, j * d:(j + 1) * d]
    for b in range(B):
        S = np.linalg.inv(np_btd.to_dense(diag[b], sub[b], symmetric=True))
        X = S @ np_btd.to_dense(dPd[b], dPs[b], symmetric=True) @ S
        covs.append(np.stack([blk(S, t, t) for t in range(T)]))
        subs.append(np.stack([blk(S, t + 1, t) for t in range(T - 1)]))
        Xd.append(np.stack([blk(X, t, t) for t in range(T)]))
        Xs.append(np.stack([blk(X, t + 1, t) for t in range(T - 1)]))
    args = (dev(np.stack(covs)), dev(np.stack(subs)), dev(dPd), dev(dPs))
    gd, gs = tape.band_of_sigma_dP_sigma(*args)
    assert_close(host(gd), np.stack(Xd), rtol=1e-8)
    assert_close(host(gs), np.stack(Xs), rtol=1e-8)
    os.environ["VIDP_TAPE_TORCH_SCAN"] = "1"
    try:
        td, ts = tape.band_of_sigma_dP_sigma(*args)
    finally:
        del os.environ["VIDP_TAPE_TORCH_SCAN"]
    assert_close(host(gd), host(td), rtol=1e-9)
    assert_close(host(gs), host(ts), rtol=1e-9)


def test_wide_band_long_chain_and_failure_report(amd, rng):
    """A chain of 3 000 nodes at d = 20 (55 segments per recurrence) against the torch scans, and ArithmeticError for a marginal
    covariance that is not positive definite."""
    from vidp_amd import tape
    B, T, d = 1, 3000, 20
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    plan = amd.Plan(B, T, d)
    f = plan.factor(plan.pack(amd.SYM, dev(diag)), plan.pack(amd.FULL, dev(sub)), None, want_logdet=False)
    s = plan.selinv(f["L"], f["G"], None, want_sub=True)
    cov, csub = plan.unpack(amd.SYM, s["Sig"]), plan.unpack(amd.FULL, s["Sub"], T - 1)
    dPd = rng.normal(size=(B, T, d, d))
    dPd = dev(dPd + np.swapaxes(dPd, -1, -2))
    dPs = dev(rng.normal(size=(B, T - 1, d, d)))
    gd, gs = tape.band_of_sigma_dP_sigma(cov, csub, dPd, dPs)
    os.environ["VIDP_TAPE_TORCH_SCAN"] = "1"
    try:
        td, ts = tape.band_of_sigma_dP_sigma(cov, csub, dPd, dPs)
    finally:
        del os.environ["VIDP_TAPE_TORCH_SCAN"]
    assert_close(host(gd), host(td), rtol=1e-9)
    assert_close(host(gs), host(ts), rtol=1e-9)
    bad = cov.clone()
    bad[0, 1234] = -bad[0, 1234]
    with pytest.raises(ArithmeticError):
        tape.band_of_sigma_dP_sigma(bad, csub, dPd, dPs)


@pytest.mark.parametrize("B,T,d,R0", [(1, 1, 1, 0), (3, 2, 2, 0), (2, 37, 3, 4), (5, 130, 6, 8), (1, 700, 8, 5), (70, 20, 4, 0), (2, 5000, 6, 0)])
def test_congruence_scan_kernel(amd, rng, B, T, d, R0):
    """mfgm_congruence_scan (X_t = Phi_t X_{t-1} Phi_t^T + Q_t, X_{-1} = 0; segment maps, their scan, final sweep) against the sequential
    recurrence in NumPy, on contractive and on mildly expanding transitions, ragged last segments and chains shorter than a segment."""
    Phi = rng.normal(size=(B, T, d, d)) * (0.9 / np.sqrt(d))
    Q = rng.normal(size=(B, T, d, d))
    Q = Q @ np.swapaxes(Q, -1, -2) + 0.1 * np.eye(d)
    ref = np.zeros_like(Q)
    X = np.zeros((B, d, d))
    for t in range(T):
        X = Phi[:, t] @ X @ np.swapaxes(Phi[:, t], -1, -2) + Q[:, t]
        ref[:, t] = X
    plan = amd.Plan(B, T, d, R0=R0)
    got = plan.unpack(amd.SYM, plan.congruence_scan(plan.pack(amd.FULL, dev(Phi)), plan.pack(amd.SYM, dev(Q))))
    np.testing.assert_allclose(host(got), ref, rtol=1e-10, atol=1e-12)


def test_tape_exact_backward_agrees_with_richardson(amd, rng):
    """The exact backward of theta -> eta against the round-2 Richardson evaluation on a well-conditioned chain (where that one is
    accurate): 1e-7 on every block, and the linear part -- which the difference quotient only reached to 1e-4 -- tighter than that."""
    import torch
    from vidp_amd import tape
    B, T, d = 2, 40, 3
    prm = [dev(a) for a in random_ssm_params(rng, (B,), T, d)]
    w = [dev(rng.normal(size=s)) for s in ((B, T, d), (B, T, d, d), (B, T - 1, d, d))]

    def grads(flag):
        tape.NaturalsToExpectations.richardson = flag
        try:
            q = tape.TapeSSM(*[p.clone().requires_grad_(True) for p in prm])
            e = q.expectations()
            loss = sum((a * b).sum() for a, b in zip(e, w)) + (e[1] ** 2).sum()
            return [host(g) for g in torch.autograd.grad(loss, q.parameters)]
        finally:
            tape.NaturalsToExpectations.richardson = False
    for a, b in zip(grads(False), grads(True)):
        assert_close(a, b, rtol=1e-6, scale_atol=1e-7)


@pytest.mark.parametrize("d", [3, 12])
def test_tape_backward_with_unused_outputs(amd, rng, d):
    """A loss that uses only some of (eta_lin, eta_diag, eta_sub): autograd hands the backward None for the others and the Fisher-vector
    product skips their work (no band for a means-only loss) -- same gradients as with explicit zero cotangents, for a packed (d = 3) and
    a wide (d = 12) plan."""
    import torch
    from vidp_amd import tape
    B, T = 2, 30
    prm = [dev(a) for a in random_ssm_params(rng, (B,), T, d)]
    w = [dev(rng.normal(size=s)) for s in ((B, T, d), (B, T, d, d), (B, T - 1, d, d))]
    for used in ((0,), (1,), (2,), (0, 2)):
        def grads(explicit):
            q = tape.TapeSSM(*[p.clone().requires_grad_(True) for p in prm])
            e = q.expectations()
            loss = sum((e[k] * w[k]).sum() for k in used)
            if explicit:      # every output takes part, the unused ones with weight zero
                loss = loss + sum((e[k] * torch.zeros_like(w[k])).sum() for k in range(3) if k not in used)
            return [host(g) for g in torch.autograd.grad(loss, q.parameters)]
        for a, b in zip(grads(False), grads(True)):
            assert_close(a, b, rtol=1e-10, scale_atol=1e-11)


@pytest.mark.parametrize("kname", ["m12", "sum"])
def test_cvi_classic_elbo_site_gradient_vanishes_at_optimum(amd, rng, kname):
    """KA7's third clause (reference tests/integration/models/test_variational_cvi.py:93-110, kernel and likelihood frozen at :58-59):
    after one site update with learning rate 1 and a Gaussian likelihood the gradient of classic_elbo with respect to the site
    parameters is zero and a further update leaves the ELBO where it is; away from the optimum the same tape gradient matches central
    differences of classic_elbo() evaluated through the ordinary (HIP, tape-free) path."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    mk = {"m12": (lambda m: m.Matern12(2.0, 2.25)), "sum": (lambda m: m.Sum([m.Matern32(1.1, 0.7), m.Matern12(0.5, 1.2)]))}[kname]
    t = np.sort(rng.uniform(0, 4, size=8))
    y = np.cos(3 * t)[:, None] + 0.1 * rng.normal(size=(8, 1))
    g = CVIGaussianProcess((dev(t), dev(y)), mk(K), Gaussian(1.0), learning_rate=1.0)
    g.update_sites()
    optim = float(g.elbo())
    g.update_sites()
    np.testing.assert_allclose(float(g.elbo()), optim, atol=1e-9)
    e, (n1, n2) = g.classic_elbo_tape()
    np.testing.assert_allclose(float(e.detach()), float(g.classic_elbo()), rtol=1e-9)
    g1, g2 = torch.autograd.grad(e, [n1, n2])
    np.testing.assert_allclose(host(g1), 0.0, atol=2e-8)
    np.testing.assert_allclose(host(g2), 0.0, atol=2e-8)
    # away from the optimum: one damped step
    h = CVIGaussianProcess((dev(t), dev(y)), mk(K), Gaussian(0.3), learning_rate=0.4)
    h.update_sites()
    e, (n1, n2) = h.classic_elbo_tape()
    g1, g2 = (host(x) for x in torch.autograd.grad(e, [n1, n2]))
    assert np.abs(g1).max() > 1e-2
    base1, base2 = h.sites.nat1.clone(), h.sites.nat2.clone()
    for which, idx, got in ((1, (3, 0), g1[3, 0]), (2, (5, 0, 0), g2[5, 0, 0]), (1, (0, 0), g1[0, 0])):
        def val(eps):
            h.sites.nat1, h.sites.nat2 = base1.clone(), base2.clone()
            (h.sites.nat1 if which == 1 else h.sites.nat2)[idx] += eps
            return float(h.classic_elbo())
        step = 1e-4
        fd = (8 * (val(step / 2) - val(-step / 2)) - (val(step) - val(-step))) / (6 * step)
        # (the Matern-3/2 component loses digits to cancellation in Q = Pinf - A Pinf A^T, as in KA7 above: the difference quotient of the
        #  ordinary path carries that noise divided by the step)
        np.testing.assert_allclose(got, fd, rtol=1e-6 if kname == "m12" else 1e-4, atol=1e-8)


@pytest.mark.parametrize("kname", ["m32", "m52", "sum"])
def test_cvi_classic_elbo_kernel_hyperparameter_gradient(amd, rng, kname):
    """The gradient of classic_elbo with respect to the KERNEL's hyper-parameters through the tape (the reference differentiates its
    models through the banded ops with a GradientTape over every trainable variable, tests/integration/models/test_variational_cvi.py:93-110;
    its own test freezes the kernel, so the known answer used here is ours): with a Gaussian likelihood the optimal sites (y / s2, -1/2 / s2)
    do not depend on the kernel and classic_elbo at them IS the GPR log marginal likelihood for every hyper-parameter value, so
    d classic_elbo / d (lengthscale, variance) at fixed optimal sites = the derivative of the oracle's gpr_log_likelihood (fourth-order
    difference quotient)."""
    import torch
    from oracle import np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    hyp = {"m32": [(1.1, 0.7)], "m52": [(0.9, 1.3)], "sum": [(1.4, 0.6), (0.5, 1.2)]}[kname]

    def mk(mod, h):
        if kname == "m32":
            return mod.Matern32(*h[0])
        if kname == "m52":
            return mod.Matern52(*h[0])
        return mod.Sum([mod.Matern32(*h[0]), mod.Matern12(*h[1])])
    # evenly spaced points: with gaps of ~0.5 lengthscales the prior's natural parameters are O(10); at the tiny random gaps of the other
    # CVI tests they reach 1e7 and the O(1) total derivative is what is left of terms that size cancelling (3e-5 relative on the
    # Matern-3/2 case -- the conditioning of differentiating in natural parameters, in the reference's tape as much as here)
    t = np.linspace(0.0, 5.0, 10) + 0.05 * rng.uniform(-1, 1, size=10)
    y = np.sin(2 * t)[:, None] + 0.1 * rng.normal(size=(10, 1))
    noise = 0.4
    g = CVIGaussianProcess((dev(t), dev(y)), mk(K, hyp), Gaussian(noise), learning_rate=1.0)
    g.update_sites()
    elbo, leaves = g.classic_elbo_tape_hyper()
    ref = lambda h: np_models.gpr_log_likelihood(t, y, mk(np_kernels, h), noise)
    np.testing.assert_allclose(float(elbo.detach()), ref(hyp), rtol=1e-8)
    flat = [leaves] if isinstance(leaves, dict) else leaves
    names = [(c, n) for c in range(len(flat)) for n in ("lengthscale", "variance")]
    grads = torch.autograd.grad(elbo, [flat[c][n] for c, n in names])
    for (c, n), gr in zip(names, grads):
        def at(e):
            h = [list(x) for x in hyp]
            h[c][0 if n == "lengthscale" else 1] += e
            return ref([tuple(x) for x in h])
        e = 1e-3
        fd = (8 * (at(e) - at(-e)) - (at(2 * e) - at(-2 * e))) / (12 * e)
        np.testing.assert_allclose(float(gr), fd, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("kind", ["vanderpol", "vanderpol_fullq", "mlp", "doublewell_fullq"])
def test_cvi_sites_sde_coupled_drifts(amd, rng, kind):
    """The drifts that couple the state dimensions / have no polynomial form (markovflow/sde/sde.py:359-518: VanderPolOscillatorSDE,
    MLPDrift) and a NON-DIAGONAL diffusion matrix (sde_utils.py:262-359 takes the full Qp^{-1}), through CVISitesSDEQuadrature on the HIP
    quadrature kernels (csrc/mfgm_quad.h: the reference's Gauss-Hermite rules with the tape's chain rule written out):
      * against the batched-torch evaluation + autograd of the same formulas (VIDP_QUAD_TORCH=1's route): linearised prior, KL and its
        gradient with respect to the expectation parameters, 1e-9;
      * against the oracle's restatement: KL 1e-10, the gradient against a fourth-order difference quotient of the oracle's quadrature
        KL -- 1e-8 relative (floor 1e-6 of the gradient's scale: that quotient's rounding noise) for the smooth drifts (a ReLU drift keeps O(step) kinks in any difference quotient: 2e-5 there) --, and the ELBO
        over damped data / Girsanov updates and a re-linearisation."""
    import torch
    from oracle import np_sde
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDEQuadrature
    T, dt = 16, 0.05
    grid = np.arange(T) * dt
    if kind.startswith("vanderpol"):
        d = 2
        q = 0.5 * np.eye(2) if kind == "vanderpol" else np.array([[0.5, 0.12], [0.12, 0.4]])
        o_sde, g_sde = np_sde.VanderPolSDE(1.3, 0.9, q), gsde.VanderPolOscillatorSDE(1.3, 0.9, torch.from_numpy(q))
    elif kind == "doublewell_fullq":
        d = 2
        q = np.array([[0.8, -0.2], [-0.2, 0.6]])
        o_sde, g_sde = np_sde.DoubleWellSDE(q, scale=2.0, c=0.7), gsde.DoubleWellSDE(torch.from_numpy(q), scale=2.0, c=0.7)
    else:
        d = 1
        w = (rng.normal(size=(1, 3)), 0.1 * rng.normal(size=3), rng.normal(size=(3, 1)), np.zeros(1))
        o_sde, g_sde = np_sde.MLPDriftSDE(w), gsde.MLPDrift(weights=[torch.from_numpy(np.asarray(x)) for x in w])
    smooth = kind != "mlp"
    idx = np.array([3, 7, 12])
    y = rng.normal(size=(1, len(idx), d))
    cholR = 0.4 * np.eye(d)
    init = (np.zeros(d), 0.8 * np.eye(d))
    mk = lambda: CVISitesSDEQuadrature(g_sde, grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)), prior_initial_state=init)
    g, gt = mk(), mk()
    assert g.native
    gt.native = False
    gt.set_linearized_prior()
    # (exact_q: the linearised prior's process noise is q itself; the reference forms chol_q @ chol_q, sde_utils.py:173, which is q only
    #  when q is diagonal -- oracle/np_sde.linearize_sde)
    o = np_models.CVISitesSDE(o_sde, grid, idx, y[0], np_models.MultivariateGaussianLik(cholR), *init, exact_q=kind.endswith("fullq"))
    for ref_A, ref_b, tol in ((host(gt.dist_p.state_transitions)[0], host(gt.dist_p.state_offsets)[0], 1e-12), (o.dist_p.A, o.dist_p.b, 1e-9)):
        assert_close(host(g.dist_p.state_transitions)[0], ref_A, rtol=tol)
        assert_close(host(g.dist_p.state_offsets)[0], ref_b, rtol=tol)
    for m in (g, gt, o):
        m.update_data_sites(0.5)
    np.testing.assert_allclose(float(g.KL_q_p()[0]), o.KL_q_p(), rtol=1e-10)
    np.testing.assert_allclose(float(g.KL_q_p()[0]), float(gt.KL_q_p()[0]), rtol=1e-12)
    kl, (g1, gd, gs) = g.grad_kl_wrt_exp_param()
    _, (t1, td, ts) = gt.grad_kl_wrt_exp_param()
    pl = g.plan
    un = lambda m_, a, b_, c: (host(m_.plan.unpack(amd.VEC, a))[0], host(m_.plan.unpack(amd.SYM, b_))[0], host(m_.plan.unpack(amd.FULL, c, T - 1))[0])
    got, tape_ = un(g, g1, gd, gs), un(gt, t1, td, ts)
    for a_, b_ in zip(got, tape_):
        assert_close(a_, b_, rtol=1e-9, scale_atol=1e-10)
    qo = o.dist_q
    mu, cov = qo.marginals
    sub = qo.subsequent_covariances(cov)
    want = np_sde.sde_ssm_kl_grads_fd(mu, cov + mu[:, :, None] * mu[:, None, :], sub + mu[1:, :, None] * mu[:-1, None, :], o_sde, dt,
                                      init[0], init[1], eps=2e-4, richardson=True)
    for a_, b_ in zip(got, want):
        # (absolute floor: the difference quotient's own rounding noise, eps |KL| / step, up to ~8e-7 here; a larger step trades it for truncation error: the KL's logdet / inverse terms have large high derivatives)
        assert_close(a_, b_, rtol=1e-8 if smooth else 2e-5, scale_atol=1e-6 if smooth else 2e-6)
    for it in range(2):
        for m in (g, o):
            m.update_girsanov_sites(0.2)
            m.update_data_sites(0.4)
        np.testing.assert_allclose(float(g.classic_elbo()), o.classic_elbo(), rtol=1e-7 if smooth else 1e-5)
        if it == 0:
            g.relinearize()
            o.relinearize()
            np.testing.assert_allclose(float(g.classic_elbo()), o.classic_elbo(), rtol=1e-7 if smooth else 1e-5)
    g.plan.check_info()
