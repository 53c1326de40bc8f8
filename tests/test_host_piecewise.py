"""
Host tests of the piecewise-stationary kernel (vidp_amd.kernels.PiecewiseKernel, change points): the region rule, the constructor's
errors, the per-region lookups and the torch closed forms against the NumPy restatement tests/np_piecewise.py; the restatement against
the reference's two known answers (tests/integration/test_kernels.py:204-269) and against the dense-GP identities the GPU tests of
GaussianProcessRegression and predict_f use, at their bounds.  No GPU.
"""
import numpy as np
import pytest

from oracle import np_kalman, np_kernels, np_models
from tests import np_kernels_ext as E
from tests import np_piecewise as PW


def test_region_rule_at_ties_and_outside():
    """r(t) = #{c_k <= t}: a point on a change point belongs to the region after it, repeated change points skip a region, points
    before / after all change points are in the first / last region."""
    import torch
    from vidp_amd import kernels as K
    cp = [0.0, 1.0, 1.0, 2.5]
    t = np.array([[-3.0, -1e-300, 0.0, 0.5], [1.0, np.nextafter(1.0, 0.0), 2.5, 1e9]])
    want = np.array([[0, 0, 1, 1], [3, 1, 4, 4]])
    np.testing.assert_array_equal(PW.PiecewiseKernel([np_kernels.Matern12(1.0, 1.0)] * 5, cp).region(t), want)
    gk = K.PiecewiseKernel([K.Matern12(1.0, 1.0) for _ in range(5)], cp)
    np.testing.assert_array_equal(gk.split_time_indices(torch.from_numpy(t)).numpy(), want)
    np.testing.assert_array_equal(gk.change_points.numpy(), cp)
    # no change point: one region everywhere
    one = K.PiecewiseKernel([K.Matern32(1.0, 1.0)], [])
    assert one.split_time_indices(torch.from_numpy(t)).abs().max() == 0 and one.state_dim == 2


def test_constructor_errors():
    from vidp_amd import kernels as K
    m = lambda l=1.0: K.Matern32(l, 1.0)
    with pytest.raises(TypeError, match="same class"):
        K.PiecewiseKernel([m(), K.Matern52(1.0, 1.0)], [0.0])
    with pytest.raises(TypeError, match="Kernel instances"):
        K.PiecewiseKernel([m(), "matern"], [0.0])
    with pytest.raises(ValueError, match="change points need"):
        K.PiecewiseKernel([m(), m()], [0.0, 1.0])
    with pytest.raises(ValueError, match="at least one"):
        K.PiecewiseKernel([], [])
    with pytest.raises(ValueError, match="sorted"):
        K.PiecewiseKernel([m(), m(), m()], [1.0, 0.0])
    with pytest.raises(ValueError, match="jitter on a child"):
        K.PiecewiseKernel([m(), K.Matern32(1.0, 1.0, jitter=1e-6)], [0.0])
    with pytest.raises(ValueError, match="jitter on a child"):
        K.PiecewiseKernel([K.Sum([m(), K.Matern12(1.0, 1.0, jitter=1e-6)]), K.Sum([m(), K.Matern12(1.0, 1.0)])], [0.0])
    # the same class, another structure: Sums of different children, Products in another order
    with pytest.raises(ValueError, match="same structure"):
        K.PiecewiseKernel([K.Sum([m(), K.Matern12(1.0, 1.0)]), K.Sum([m(), m()])], [0.0])
    with pytest.raises(ValueError, match="same structure"):
        K.PiecewiseKernel([K.Product([m(), K.HarmonicOscillator(1.0, 1.0)]), K.Product([K.HarmonicOscillator(1.0, 1.0), m()])], [0.0])
    # equal change points are sorted; trees are admissible
    K.PiecewiseKernel([m(), m(), m()], [1.0, 1.0])
    K.PiecewiseKernel([K.Sum([m(0.5), K.Product([K.Matern12(1.0, 1.0), K.HarmonicOscillator(1.0, 1.0)])]),
                       K.Sum([m(2.0), K.Product([K.Matern12(3.0, 2.0), K.HarmonicOscillator(0.5, 2.0)])])], [0.3])


def test_models_out_of_scope_name_the_kernel():
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, PEPScalarLikelihood
    from vidp_amd.space_kernels import SquaredExponential
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    pk = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], [0.0])
    z = torch.linspace(-1.0, 1.0, 5, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="PiecewiseKernel"):
        SparsePowerExpectationPropagation(pk, z, PEPScalarLikelihood(Bernoulli()))
    with pytest.raises(NotImplementedError, match="PiecewiseKernel"):
        SpatioTemporalSparseCVI(torch.zeros((2, 1), dtype=torch.float64), z, SquaredExponential(1.0, 1.0), pk, Bernoulli())


def _pair(rng, with_means=True):
    """The same 4-region Sum(Matern52, Product(Matern12, HarmonicOscillator)) kernel (d = 5) in torch and in NumPy."""
    from vidp_amd import kernels as K
    prm = [(0.5, 1.0, 0.8, 2.0, 0.7, 0.6), (1.1, 0.4, 0.3, 1.0, 1.3, 0.9), (0.8, 2.2, 1.5, 0.5, 0.4, 1.4), (2.0, 0.7, 0.6, 1.5, 1.0, 0.5)]
    cp = [0.2, 0.9, 1.7]

    def mk(m, x, p):
        return m.Sum([m.Matern52(p[0], p[1]), x.Product([m.Matern12(p[2], p[3]), x.HarmonicOscillator(p[4], p[5])])])
    gks, oks = [mk(K, K, p) for p in prm], [mk(np_kernels, E, p) for p in prm]
    if with_means:
        for g, o in zip(gks, oks):
            for gc, oc in zip(g.kernels, o.kernels):
                mean = rng.normal(size=gc.state_dim)
                gc.set_state_mean(mean)
                oc._state_mean = mean
    return K.PiecewiseKernel(gks, cp, jitter=1e-6), PW.PiecewiseKernel(oks, cp, jitter=1e-6), gks, oks


def test_per_region_lookups_match_the_children(rng):
    import torch
    gk, ok, gks, _ = _pair(rng)
    t = rng.uniform(-1.0, 3.0, size=(2, 9))
    t[0, :3] = [0.2, 0.9, 1.7]
    r = ok.region(t)
    tt = torch.from_numpy(t)
    for got, per_child, want in ((gk.steady_state_covariances(tt), [k.steady_state_covariance for k in gks], ok.steady_state_covariance_at(t)),
                                 (gk.feedback_matrices(tt), [k.feedback_matrix for k in gks], ok.feedback_matrix_at(t)),
                                 (gk.state_means(tt), [k.state_mean for k in gks], ok.state_mean_at(t))):
        np.testing.assert_array_equal(got.numpy(), np.stack([c.numpy() for c in per_child])[r])
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-14, atol=1e-14)
    assert set(r.reshape(-1)) == {0, 1, 2, 3}
    np.testing.assert_array_equal(gk.initial_mean((2,)).numpy(), np.zeros((2, 5)))
    np.testing.assert_allclose(gk.initial_covariance(tt[:, :1]).numpy(), ok.initial_covariance_at(t[:, 0]), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(gk.initial_covariance(tt[0, :1]).numpy(), ok.initial_covariance_at(t[0, 0]), rtol=1e-14, atol=1e-14)
    np.testing.assert_array_equal(gk.generate_emission_model(tt).emission_matrix.numpy(), ok.emission_matrix(t))
    assert gk.generate_emission_model(tt).constant_matrix is not None


def test_torch_closed_forms_match_numpy(rng):
    """transition_statistics / state_offsets (the left end decides) on unordered gaps, zero gaps and gaps that cross change points."""
    import torch
    gk, ok, _, _ = _pair(rng)
    tl = rng.uniform(-1.0, 3.0, size=(3, 7))
    dt = rng.exponential(0.4, size=(3, 7))
    tl[0, :2], dt[0, :2] = [0.9, 0.9 - 1e-12], [0.0, 2.0]
    oA, oQ, ob = ok.transition_statistics_at(tl, dt)
    A, Q = gk.transition_statistics(torch.from_numpy(tl), torch.from_numpy(dt))
    scale = np.abs(ok.steady_state_covariance_at(tl)).max()
    np.testing.assert_allclose(A.numpy(), oA, rtol=0, atol=1e-13)
    np.testing.assert_allclose(Q.numpy(), oQ, rtol=0, atol=1e-13 * scale)
    np.testing.assert_allclose(gk.state_offsets(torch.from_numpy(tl), torch.from_numpy(dt)).numpy(), ob, rtol=0, atol=1e-13 * np.abs(ob).max())
    np.testing.assert_array_equal(gk.state_transitions(torch.from_numpy(tl), torch.from_numpy(dt)).numpy(), A.numpy())


def test_stationary_kernels_ignore_the_times(rng):
    """The time-aware forms of a stationary kernel are its old ones, bit for bit."""
    import torch
    from vidp_amd import kernels as K
    dt = torch.from_numpy(rng.exponential(0.4, size=(2, 6)))
    tl = torch.from_numpy(rng.normal(size=(2, 6)))
    for k in (K.Matern52(0.7, 1.3, jitter=1e-8), K.Sum([K.Matern32(0.7, 1.3), K.Matern12(1.0, 2.0)]),
              K.Product([K.Matern32(0.7, 1.3), K.HarmonicOscillator(1.0, 1.5)], jitter=1e-7)):
        for a, b in zip(k.transition_statistics_at(tl, dt), k.transition_statistics_local(dt)):
            assert torch.equal(a, b)
        assert torch.equal(k.initial_covariance(tl[0, :1]), k.initial_covariance_matrix())


def test_known_answer_shared_base():
    """Six identical Matern32(1, 1) children give the base kernel's marginals on linspace(1, 5, 100) (and its covariance function)."""
    cp = np.arange(5.0)
    pk = PW.PiecewiseKernel([np_kernels.Matern32(1.0, 1.0) for _ in range(6)], cp)
    base = np_kernels.Matern32(1.0, 1.0)
    x = np.linspace(1.0, 5.0, 100)
    mu_pk, cov_pk = pk.state_space_model(x).marginals
    mu, cov = base.state_space_model(x).marginals
    np.testing.assert_allclose(mu_pk, mu, rtol=0, atol=1e-14)
    np.testing.assert_allclose(cov_pk, cov, rtol=0, atol=1e-13)
    np.testing.assert_allclose(PW.f_covariance(pk, x), E.dense_k(base, x[:, None] - x[None, :]), rtol=0, atol=1e-12)


def test_known_answer_stitched():
    """... equals the two separately built SSMs stitched at 0."""
    ks, xs, x = PW.stitched_case()
    pk = PW.PiecewiseKernel(ks, [-1e-5])
    mu_pk, cov_pk = pk.state_space_model(x).marginals
    cov = PW.marginal_covariances(*PW.stitched_parameters(ks, xs))
    np.testing.assert_allclose(mu_pk, 0.0, rtol=0, atol=0)
    np.testing.assert_allclose(cov_pk, cov, rtol=0, atol=1e-13)
    # the first half is the first kernel's stationary state, the second half relaxes towards the second kernel's
    np.testing.assert_allclose(cov[:5], np.broadcast_to(ks[0].steady_state_covariance(), (5, 2, 2)), rtol=0, atol=1e-13)
    assert np.abs(cov[-1] - ks[0].steady_state_covariance()).max() > 0.1


def test_numpy_gpr_equals_the_dense_gp(rng):
    """The bound of the GPU test is reachable: the Kalman log marginal likelihood on the NumPy SSM equals the dense Gaussian log
    density of its f covariance plus noise at rtol 1e-9."""
    t, y, cp, prm, noise = PW.gpr_case(rng)
    pk = PW.PiecewiseKernel([np_kernels.Matern32(*p) for p in prm], cp)
    dense = PW.dense_logml(PW.f_covariance(pk, t) + noise * np.eye(t.size), y[:, 0])
    np.testing.assert_allclose(np_models.gpr_log_likelihood(t, y, pk, noise), dense, rtol=1e-9)


def test_numpy_prediction_equals_dense_conditioning(rng):
    """The bound of the GPU test is reachable: the Kalman posterior on the training grid pushed through the time-aware conditionals
    equals dense conditioning on the union grid at 1e-8, because no transition of either grid crosses a change point."""
    t, y, cp, prm, noise, tn = PW.predict_case(rng)
    pk = PW.PiecewiseKernel([np_kernels.Matern32(*p) for p in prm], cp)
    kf = np_kalman.KalmanFilter(pk.state_space_model(t), pk.emission_matrix(t), y, np.sqrt(noise) * np.eye(1))
    mu, var = PW.predict_f(kf.posterior_state_space_model(), pk, t, tn)
    om, ov = PW.dense_predict(pk, t, y, noise, tn)
    np.testing.assert_allclose(mu[:, 0], om, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(var[:, 0], ov, rtol=1e-8, atol=1e-8)
    assert len(set(pk.region(tn))) == 3 and (tn < t[0]).any() and (tn > t[-1]).any()
