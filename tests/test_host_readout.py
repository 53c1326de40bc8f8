"""CPU tests of the linear-readout likelihood (vidp_amd.likelihoods.LinearReadout, torch route) against the NumPy restatement
tests/np_readout.py and the identities of its contract, and the argument checks of mfgm_readout_site_update / mfgm_readout_obs_ve
(which run before anything touches a device)."""
import ctypes

import numpy as np
import pytest

from tests import np_readout


@pytest.fixture(scope="module")
def L():
    import vidp_amd  # noqa: F401
    from vidp_amd import likelihoods
    return likelihoods


def T(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def within(got, want, scale, what):
    err = np.abs(np.asarray(got) - want)
    assert np.all(err <= 1e-12 * scale), f"{what}: worst error / scale = {np.max(err / np.maximum(scale, 1e-300)):.3g}"


@pytest.mark.parametrize("d", [1, 3, 6, 8])
@pytest.mark.parametrize("which_o", ["one", "two", "d"])
def test_torch_route_matches_numpy(L, rng, d, which_o):
    """VE, g1, g2 at mixed kinds, offsets and ~10 % NaN entries: 1e-12 of the sum of absolute terms of each quantity."""
    o = {"one": 1, "two": 2, "d": d}[which_o]
    kinds = {"one": "b", "two": "pg", "d": "gpb"}[which_o]
    n = 400
    H, c, spec, ref = np_readout.random_readout(rng, d, o, kinds)
    lik = np_readout.torch_readout(L, H, c, spec)
    assert (lik.state_dim, lik.obs_dim, lik.uniform_site_gradient) == (d, o, False)
    mu, cov = np_readout.random_marginals(rng, n, d)
    y = np_readout.random_observations(rng, ref, mu)
    y[7] = np.nan
    (ve, g1, g2), (sv, s1, s2) = ref.all_with_scales(mu, cov, y)
    got = lik.variational_expectations(T(mu), T(cov), T(y)).numpy()
    assert got.shape == (n,)
    within(got, ve, sv, "VE")
    a1, a2 = (x.numpy() for x in lik.ve_gradients_expectation(T(mu), T(cov), T(y)))
    assert a1.shape == (n, d) and a2.shape == (n, d, d)
    within(a1, g1, s1, "g1")
    within(a2, g2, s2, "g2")
    m, v = (x.numpy() for x in lik.project(T(mu), T(cov)))
    rm, rv = ref.project(mu, cov)
    np.testing.assert_allclose(m, rm, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(v, rv, rtol=1e-12)
    # a row that is all NaN contributes exactly nothing
    assert got[7] == 0.0 and not a1[7].any() and not a2[7].any()


def test_generic_factor_takes_the_torch_route(L, rng):
    """A ScalarQuadratureLikelihood that is not one of the native kinds: same numbers as the Poisson it restates, native_kinds False."""
    d, n = 3, 100
    H = rng.normal(size=(2, d))
    po = L.Poisson(0.7)
    a = L.LinearReadout(H, [L.Gaussian(0.4), po])
    b = L.LinearReadout(H, [L.Gaussian(0.4), L.ScalarQuadratureLikelihood(po.log_prob)])
    assert a.native_kinds and not b.native_kinds
    mu, cov = np_readout.random_marginals(rng, n, d)
    cov = 0.2 * cov
    y = np.stack([rng.normal(size=n), rng.poisson(2.0, size=n)], -1).astype(np.float64)
    np.testing.assert_allclose(b.variational_expectations(T(mu), T(cov), T(y)).numpy(),
                               a.variational_expectations(T(mu), T(cov), T(y)).numpy(), rtol=1e-11)
    for x, z in zip(b.ve_gradients_expectation(T(mu), T(cov), T(y)), a.ve_gradients_expectation(T(mu), T(cov), T(y))):
        np.testing.assert_allclose(x.numpy(), z.numpy(), rtol=1e-10, atol=1e-12)
    with pytest.raises(ValueError):
        L.LinearReadout(np.zeros((9, 3)), po)
    with pytest.raises(ValueError):
        L.LinearReadout(H, [po])
    with pytest.raises(TypeError):
        L.LinearReadout(H, object())


@pytest.mark.parametrize("kinds", ["g", "p", "b", "gpb"])
def test_gradients_are_central_differences_of_the_restatement(rng, kinds):
    """(g1, g2) = gradient_transformation_mean_var_to_expectation of (dVE/dmu, dVE/dSigma), the derivatives taken as central differences
    of the restatement's own VE(mu, Sigma) (for Bernoulli VE is the 20-point rule, so the rule is what is differenced).  Step 1e-5:
    truncation ~ 1e-10 of the third derivative, rounding ~ 1e-16 |VE| / 1e-5; 1e-6 relative (to the largest entry of the observation's
    gradient)."""
    d, o, n, h = 3, 3, 12, 1e-5
    H, c, spec, ref = np_readout.random_readout(rng, d, o, kinds)
    mu, cov = np_readout.random_marginals(rng, n, d)
    y = np_readout.random_observations(rng, ref, mu)
    g1, g2 = ref.grads_expectation(mu, cov, y)
    ve = lambda m, S: ref.variational_expectations(m, S, y)
    dmu, dS = np.zeros((n, d)), np.zeros((n, d, d))
    for r in range(d):
        e = np.zeros(d)
        e[r] = h
        dmu[:, r] = (ve(mu + e, cov) - ve(mu - e, cov)) / (2 * h)
        for q in range(d):
            E = np.zeros((d, d))
            E[r, q] += 0.5 * h
            E[q, r] += 0.5 * h
            dS[:, r, q] = (ve(mu, cov + E) - ve(mu, cov - E)) / (2 * h)
    f1 = dmu - 2.0 * (dS @ mu[..., None])[..., 0]
    for i in range(n):
        np.testing.assert_allclose(g2[i], dS[i], rtol=1e-6, atol=1e-6 * np.abs(dS[i]).max())
        np.testing.assert_allclose(g1[i], f1[i], rtol=1e-6, atol=1e-6 * max(np.abs(f1[i]).max(), np.abs(dmu[i]).max()))


@pytest.mark.parametrize("d", [1, 3, 6])
def test_identity_readout_is_the_multivariate_gaussian(L, rng, d):
    """H = I, every factor Gaussian with variance s^2: MultivariateGaussian(s I)."""
    s, n = 0.6, 50
    import math
    import torch
    lik = L.LinearReadout(np.eye(d), L.Gaussian(s * s))
    # MultivariateGaussian's constructor inverts its factor with the device solver; for s I the inverse is known, so the object is
    # assembled by hand here and its own variational_expectations / ve_gradients_expectation run on the host (tests/test_gpu_readout.py
    # repeats the comparison with the constructed object)
    mvn = object.__new__(L.MultivariateGaussian)
    mvn._chol, mvn.obs_dim, mvn.inv_covariance, mvn._g_cache = T(s * np.eye(d)), d, T(np.eye(d) / (s * s)), None
    mvn.log_det_chol = torch.tensor(d * math.log(s), dtype=torch.float64)
    mu, cov = np_readout.random_marginals(rng, n, d)
    y = rng.normal(size=(n, d))
    np.testing.assert_allclose(lik.variational_expectations(T(mu), T(cov), T(y)).numpy(),
                               mvn.variational_expectations(T(mu), T(cov), T(y)).numpy(), rtol=1e-12)
    for a, b in zip(lik.ve_gradients_expectation(T(mu), T(cov), T(y)), mvn.ve_gradients_expectation(T(mu), T(cov), T(y))):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=1e-15)


def test_predictions_match_numpy(L, rng):
    d, o, n = 4, 3, 60
    H, c, spec, ref = np_readout.random_readout(rng, d, o, "gpb")
    lik = np_readout.torch_readout(L, H, c, spec)
    mu, cov = np_readout.random_marginals(rng, n, d)
    y = np_readout.random_observations(rng, ref, mu)
    for a, b in zip(lik.predict_mean_and_var(T(mu), T(cov)), ref.predict_mean_and_var(mu, cov)):
        assert a.shape == (n, o)
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-12)
    lp = lik.predict_log_density(T(mu), T(cov), T(y)).numpy()
    assert lp.shape == (n,)
    np.testing.assert_allclose(lp, ref.predict_log_density(mu, cov, y), rtol=1e-11, atol=1e-13)


def test_torch_route_is_differentiable(L, rng):
    """Autograd through variational_expectations gives the gradients ve_gradients_expectation maps to the expectation parameters."""
    import torch
    d, o, n = 3, 3, 20
    H, c, spec, ref = np_readout.random_readout(rng, d, o, "gpb")
    lik = np_readout.torch_readout(L, H, c, spec)
    mu, cov = np_readout.random_marginals(rng, n, d)
    y = T(np_readout.random_observations(rng, ref, mu))
    m, S = T(mu).requires_grad_(True), T(cov).requires_grad_(True)
    gm, gS = torch.autograd.grad(lik.variational_expectations(m, S, y).sum(), [m, S])
    g1, g2 = lik.ve_gradients_expectation(m.detach(), S.detach(), y)
    np.testing.assert_allclose(gS.numpy(), g2.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose((gm - 2.0 * (gS @ m.detach()[..., None])[..., 0]).numpy(), g1.numpy(), rtol=1e-10, atol=1e-12)


def test_models_keep_state_and_observation_dimension_apart(L):
    """The constructor's bookkeeping needs no device: repeated observation times raise before anything is allocated."""
    import torch
    from vidp_amd.variational_cvi_sde import CVISitesSSM
    lik = L.LinearReadout(np.ones((1, 2)), L.Poisson())
    grid = np.arange(10) * 0.1
    with pytest.raises(ValueError, match="repeat"):
        CVISitesSSM(None, grid, (grid[[2, 5, 5]], torch.zeros((1, 3, 1), dtype=torch.float64)), lik)


# ---- argument checks of the two entry points (no GPU: every case returns before a launch) --------------------------------------------
def _readout(amd, d=3, o=2, kinds=(3, 2), params=(0.5, 1.0)):
    rd = amd._lib.Readout()
    rd.o, rd.d = o, d
    for j, (k, p) in enumerate(zip(kinds, params)):
        rd.kind[j], rd.param[j] = k, p
    for k in range(o * d):
        rd.H[k] = 0.1 * (k + 1)
    return rd


def test_argument_checks_need_no_gpu():
    import vidp_amd as amd
    lib = amd._lib.load()
    h, hw = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.mfgm_plan_create(2, 100, 3, 0, 0, ctypes.byref(h)) == 0
    assert lib.mfgm_plan_create(2, 100, 16, 0, 0, ctypes.byref(hw)) == 0
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)      # stands for a device pointer: no call below gets as far as using it

    def update(plan, rd, n=4, lr=0.5, gathered=0, ptrs=None):
        a = [p] * 8 if ptrs is None else ptrs      # mu, Sig, node_ids, y, theta_lin, theta_diag, sites_vec, sites_sym
        return lib.mfgm_readout_site_update(plan, ctypes.byref(rd), a[0], a[1], gathered, a[2], n, a[3], a[4], a[5], a[6], a[7], lr, None)

    def ve(plan, rd, n_per=4, ptrs=None):
        a = [p] * 5 if ptrs is None else ptrs      # mu, Sig, node_ids, y, ve
        return lib.mfgm_readout_obs_ve(plan, ctypes.byref(rd), a[0], a[1], a[2], n_per, a[3], None, None, a[4], None)

    good = _readout(amd)
    bad = [(hw, _readout(amd, d=16)),                                   # wide plan
           (h, _readout(amd, o=0, kinds=(), params=())),                # o outside 1 .. 8
           (h, _readout(amd, o=9)),
           (h, _readout(amd, d=4)),                                     # readout.d != plan d
           (h, _readout(amd, kinds=(3, 7))),                            # unknown kind
           (h, _readout(amd, kinds=(0, 2))),
           (h, _readout(amd, kinds=(1, 2), params=(0.5, 1.0))),         # jitter outside [0, 1/2)
           (h, _readout(amd, kinds=(1, 2), params=(-1e-3, 1.0))),
           (h, _readout(amd, kinds=(3, 2), params=(0.5, 0.0))),         # bin size <= 0
           (h, _readout(amd, kinds=(3, 2), params=(0.0, 1.0))),         # variance <= 0
           (h, _readout(amd, kinds=(3, 2), params=(float("nan"), 1.0)))]
    for plan, rd in bad:
        assert update(plan, rd) == 1
        assert ve(plan, rd) == 1
        assert update(plan, rd, n=0) == 1 and ve(plan, rd, n_per=0) == 1      # a bad description is reported even without observations
    for lr in (-0.1, 1.5, float("nan")):
        assert update(h, good, lr=lr) == 1
    assert update(h, good, gathered=2) == 1
    assert update(h, good, n=-1) == 1 and ve(h, good, n_per=-1) == 1
    for k in range(8):
        assert update(h, good, ptrs=[None if i == k else p for i in range(8)]) == 1
    for k in range(5):
        assert ve(h, good, ptrs=[None if i == k else p for i in range(5)]) == 1
    assert lib.mfgm_readout_site_update(None, ctypes.byref(good), p, p, 0, p, 4, p, p, p, p, p, 0.5, None) == 1
    assert lib.mfgm_readout_obs_ve(h, None, p, p, p, 4, p, None, None, p, None) == 1
    # no observations: a no-op that returns 0, with nothing to point to
    assert update(h, good, n=0, ptrs=[None] * 8) == 0
    assert ve(h, good, n_per=0, ptrs=[None] * 5) == 0
    for lr in (0.0, 1.0):
        assert update(h, good, n=0, lr=lr, ptrs=[None] * 8) == 0
    lib.mfgm_plan_destroy(h)
    lib.mfgm_plan_destroy(hw)


def test_descriptor_restates_the_likelihood(L):
    import vidp_amd as amd
    H = np.arange(6.0).reshape(2, 3)
    lik = L.LinearReadout(H, [L.Gaussian(0.25), L.Bernoulli(2e-3)], offset=[0.5, -1.0])
    rd = lik.descriptor()
    assert ctypes.sizeof(amd._lib.Readout) == 8 + 32 + 8 * (8 + 8 + 64)
    assert (rd.o, rd.d, list(rd.kind)[:2], list(rd.param)[:2], list(rd.offset)[:2]) == (2, 3, [3, 1], [0.25, 2e-3], [0.5, -1.0])
    assert list(rd.H)[:6] == list(H.reshape(-1))
